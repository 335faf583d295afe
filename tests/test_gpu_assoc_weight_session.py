"""A rows session with slam_pf_assoc_weight_set against the frame loop of tests/_assoc_weight_spec.py over the twelve frames of
tests/_pipeline_scenes.py, bit for bit and frame by frame — log-weights, ancestors, poses, map rows, evidence, the miss counts and
the terms — under the three noise forms, every form of the evidence stage and none, merging on and off, constants changed and the
switch turned off and on in mid-run, a frame without a hand-over and frames a gated session kept; with the constants at 0 every
launch counter but the stage's own is the switch-off session's; what the switch refuses; and slam_pf_main --assoc-weight."""
import subprocess
import sys

import numpy as np
import pytest
import torch

import _assoc_weight_scenes as WS
import _detect_spec as D
import _pipeline_scenes as SC
import test_gpu_pipeline_session as TP
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
N, L, FRAMES = SC.N, SC.L, SC.FRAMES
world = TP.world


def open_session(world, kw, new_gate=None):
    e, ses = TP.open_session(world, kw)
    if new_gate is not None:                    # the gates of this run, under the same noise form; nothing else moves
        ses.assoc_set(SC.GATE, new_gate, True)
    return e, ses


def weight_frame(ses, w, label, pruning):
    missed, terms = ses.assoc_weight_view()
    assert (missed is not None) == bool(pruning), f"{label}: the miss view"
    if w["terms"] is not None:
        assert np.array_equal(bits(TP.host(terms)), bits(w["terms"])), f"{label}: terms"
        if pruning:
            assert np.array_equal(TP.host(missed), w["missed"]), f"{label}: missed"


@pytest.mark.parametrize("name", list(WS.SESSIONS))
def test_session_equals_the_loop(world, name):
    kw = WS.SESSIONS[name]
    aw = kw["assoc_weight"]
    first = {k: v for k, v in kw.items() if k not in ("assoc_weight", "new_gate")}
    e, ses = open_session(world, first, kw.get("new_gate"))
    fov = ses.fov_view()["bounds"] if kw.get("fov") else None
    want = WS.reference(world, name, fov)
    assert any(w["stats"] is not None and w["stats"][:, 1].any() for w in want) and any(w["terms"] is not None and w["terms"].any() for w in want)
    if kw.get("prune"):
        assert any(w["missed"] is not None and w["missed"].any() for w in want)
    if kw.get("ess"):
        assert not all(w["resampled"] for w in want) and any(w["resampled"] for w in want)
    c0, stage0, now, ran = TP.counters(e), e.assoc_weight_count(), None, 0
    for f in range(FRAMES):
        c = aw(f) if callable(aw) else aw
        if c != now:
            ses.assoc_weight_set(*(c or (0.0, 0.0, 0.0)), on=c is not None)
            now = c
        det = kw.get("detector") or kw["detections"](f)
        if det is None:
            e.scan_upload(*SC.SCANS[f])
            ses.step(0, SC.DP, False)
        else:
            TP.hand_over(e, f, kw)
            ses.step(0, SC.DP, True)
            ran += c is not None
        g = TP.frame(e, ses, first)
        label = f"{name}: frame {f}"
        if det is None:
            for k in ("logw", "anc", "pose", "map"):
                assert np.array_equal(bits(g[k]), bits(want[f][k])), f"{label}: {k}"
            assert np.array_equal(g["ev"], want[f]["ev"]), f"{label}: evidence"
        else:
            TP.compare(g, want[f], label)
            if c is not None:
                weight_frame(ses, want[f], label, kw.get("prune"))
    assert e.assoc_weight_count() - stage0 == ran
    observing = sum(1 for f in range(FRAMES) if kw.get("detector") or kw["detections"](f) is not None)
    assert TP.advance(e, c0) == TP.expected(first, observing)
    ses.close()
    e.close()


def test_zero_constants_move_no_other_counter(world):
    kw = SC.COMBOS["whole pipeline"]
    fov, moved = None, []
    for on in (False, True):
        e, ses = TP.open_session(world, kw)
        fov = ses.fov_view()["bounds"]
        if on:
            ses.assoc_weight_set(0.0, 0.0, 0.0)
        c0 = TP.counters(e)
        frames = []
        for f in range(4):
            TP.hand_over(e, f, kw)
            ses.step(0, SC.DP, True)
            frames.append(TP.frame(e, ses, kw))
        moved.append((TP.advance(e, c0), e.assoc_weight_count(), frames))
        ses.close()
        e.close()
    (c_off, s_off, f_off), (c_on, s_on, f_on) = moved
    assert c_off == c_on and s_off == 0 and s_on == 4
    want = SC.reference(world, "whole pipeline", fov)
    for f in range(4):
        TP.compare(f_off[f], want[f], f"off: frame {f}")
        TP.compare(f_on[f], want[f], f"on with zeros: frame {f}")


def test_refusals(world):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))

    def refused(ses, *args, words):
        c0, s0 = TP.counters(e), e.assoc_weight_count()
        with pytest.raises(pkg.SlamError) as err:
            ses.assoc_weight_set(*args)
        assert err.value.status == -2 and all(w in str(err.value) for w in words), str(err.value)
        assert TP.counters(e) == c0 and e.assoc_weight_count() == s0

    ses = pkg.PfSession(e, N, L, map_layout="rows", **SC.KW)
    refused(ses, -1.0, -1.0, -1.0, words=("association",))           # association never switched on
    with pytest.raises(pkg.SlamError) as err:
        ses.assoc_weight_view()
    assert err.value.status == -4
    ses.assoc_weight_set(-1.0, -1.0, -1.0, on=False)                   # off is always accepted
    ses.assoc_set(SC.GATE, SC.NEW_GATE, True)
    for bad in (1e-30, 1.0, float("nan"), float("inf"), float("-inf")):
        for slot in range(3):
            c = [-1.0, -1.0, -1.0]
            c[slot] = bad
            refused(ses, *c, words=("finite", "<= 0"))
    ses.assoc_weight_set(-1.0, -0.0, 0.0)
    ses.assoc_set(0.0)                                                 # ... cleared with the association, like the other switches
    refused(ses, -1.0, -1.0, -1.0, words=("association",))
    ses.close()
    split = pkg.PfSession(e, N, L, map_layout="split", **SC.KW)
    refused(split, -1.0, -1.0, -1.0, words=("association",))
    split.close()
    group = pkg.LocalGroup(1)
    comm = pkg.Comm.local(e, group, 0)
    sharded = pkg.PfSession(e, N, L, map_layout="rows", comm=comm, **SC.KW)
    refused(sharded, -1.0, -1.0, -1.0, words=("association",))
    sharded.close()
    comm.close()
    group.close()
    e.close()


def write_dataset(path):
    """The pipeline scene as the program reads it: one line of 1079 ranges per frame (a sensor that moves, objects that come, go,
    block and walk)."""
    path.write_text("".join(",".join(f"{v:.6f}" for v in np.hypot(bx.astype(np.float64), by.astype(np.float64))) + "\n" for bx, by in SC.SCANS))


HOST_L, HOST_N, HOST_SEED = 8, 256, 3
HOST_ASSOC, HOST_PRUNE, HOST_DETECT = (9.21, 50.0), (1, 1, 3, 10.0), dict(jump=0.3, guard=1.0, max_width=0.5, max_range=20.0, min_points=3,
                                                                       max_points=40, wrap=0)


def python_run(orc, csv, consts):
    """What slam_pf_main does with `--landmarks HOST_L --assoc --prune --detect [--assoc-weight consts]`, from Python: the front
    end's pieces are the oracle's (pinned bit for bit on the C front end by test_host_frontend.py), the session is the package's.
    -> (pose log, landmark file, [created, dropped, missed, dropped - missed]: whether it differs between particles in some
    frame)."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.cosf.restype = libm.sinf.restype = ctypes.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [ctypes.c_float]
    pkg = load_package()
    ang = orc.beam_angles(-2.351831, 0.004363, 1079)
    frames = [np.array([float(v) for v in ln.split(",") if v.strip()], F) for ln in csv.read_text().splitlines()]
    e = pkg.Engine(0)
    ses = pkg.PfSession(e, HOST_N, HOST_L, map_layout="rows", seed=HOST_SEED, sigma=(0.01, 0.01, 0.002), meas_var=0.01, score_gain=0.25)
    ses.assoc_set(*HOST_ASSOC, True)
    ses.prune_set(*HOST_PRUNE)
    if consts is not None:
        ses.assoc_weight_set(*consts)
    ses.detect_set(**HOST_DETECT)
    pose, prev = np.zeros(3, F), np.zeros(3, F)
    bx, by = orc.clean_scan(frames[0], ang)
    map_x, map_y = orc.transform(bx, by, pose)
    map_pose = pose.copy()
    ses.reset(pose)
    updated, log, spread = True, [], [False] * 4
    for k in range(1, len(frames)):
        log.append(f"scan {k + 1}\n")
        bx, by = orc.clean_scan(frames[k], ang)
        e.scan_upload(bx, by)
        wx = None
        if updated:
            wx, wy = orc.transform(bx, by, pose)
            lx, ly = orc.local_map(map_x, map_y, wx, wy, 1.0)
            for slot, (pixel, ld) in enumerate(((0.2, 200), (0.1, 400))):
                grid, m = orc.rasterise(lx, ly, pixel, ld)
                e.grid_upload(slot, grid, pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y), 10.0)
        dp = (pose - prev).astype(F) if k > 1 else np.zeros(3, F)
        ses.step(1, dp, True)
        best = ses.mean(float(F(pose[2] + dp[2])))
        if consts is not None:
            st = TP.host(ses.assoc_view()["stats"])
            ms = TP.host(ses.assoc_weight_view()[0])
            for j, c in enumerate((st[:, 1], st[:, 2], ms, st[:, 2] - ms)):
                spread[j] = spread[j] or bool(c.min() != c.max())
        prev, pose = pose, best.astype(F)
        if abs(F(pose[0] - map_pose[0])) > F(0.3) or abs(F(pose[1] - map_pose[1])) > F(0.3) or abs(F(pose[2] - map_pose[2])) > F(0.0872665):
            updated = True
            if wx is None:
                wx, wy = orc.transform(bx, by, pose)
            hits, nhits = e.pose_hits(1, float(pose[0]), float(pose[1]), libm.cosf(float(pose[2])), libm.sinf(float(pose[2])))
            keep = np.nonzero(hits[:nhits] > 1.5)[0]
            map_x, map_y = np.concatenate([map_x, wx[keep]]), np.concatenate([map_y, wy[keep]])
            map_pose = pose.copy()
        else:
            updated = False
        log.append("pose = %f  %f  %f\n" % tuple(float(v) for v in pose))
    bp = ses.best()[0]
    px = ses.poses()
    same = np.nonzero((px[0] == bp[0]) & (px[1] == bp[1]) & (px[2] == bp[2]))[0]
    row = ses.map_rows([int(same[0]) if len(same) else 0])[0]
    lm = "".join("%f,%f\n" % (float(row[0, l]), float(row[1, l])) for l in range(HOST_L) if not (row[2, l] < 0))
    ses.close()
    e.close()
    return "".join(log), lm, spread


# In this scene a detection no landmark takes is dropped where a band lies between the gates and starts a landmark where none does,
# so no one run has all three counts differ between particles; two runs have each count differ in one of them, misses in both:
# name -> (slots, new_gate, the counts that must differ between particles in some frame: created, dropped, missed)
HOST_RUNS = {"a band between the gates": (8, 50.0, (False, True, True)), "no band": (10, 9.21, (True, False, True))}
HOST_CONSTS = (-4.0, -9.0, -0.5)


@pytest.mark.parametrize("name", list(HOST_RUNS))
def test_host_program_equals_a_session_driven_from_python(orc, tmp_path, monkeypatch, name):
    """slam_pf_main --assoc-weight on a moving sensor: its pose log and its --landmarks-out are those of a session driven from
    Python on the same frames with the same three constants — and not those of the switch off, nor of the constants in another
    order wherever that order can show: where it gives a count that differs between particles another constant.  (In the run with
    a band every detection in the band leaves the landmark it nearly matched without a hit: dropped and missed may move together,
    and then only the SUM of their two constants shows there — their places are told apart by the run without a band.)"""
    slots, new_gate, must = HOST_RUNS[name]
    monkeypatch.setattr(sys.modules[__name__], "HOST_L", slots)
    monkeypatch.setattr(sys.modules[__name__], "HOST_ASSOC", (9.21, new_gate))
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv, lm = tmp_path / "scene.csv", tmp_path / "landmarks.csv"
    write_dataset(csv)
    args = [str(exe), str(csv), str(len(SC.SCANS)), "1079", str(tmp_path / "map.csv"), str(HOST_N), str(HOST_SEED), "--landmarks", str(slots),
            "--assoc", "9.21", f"{new_gate:g}", "--prune", "1", "1", "3", "10", "--assoc-weight"] + [f"{c:g}" for c in HOST_CONSTS] + \
           ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)]
    r = subprocess.run(args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    program = (r.stdout, lm.read_text())
    want = python_run(orc, csv, HOST_CONSTS)
    print("counts that differ between particles (created, dropped, missed):", want[2])
    assert all(w or not m for w, m in zip(want[2][:3], must)), f"a count that should differ between particles does not: {want[2]}"
    tied = not want[2][3]
    assert program[0] == want[0], "pose log"
    assert program[1] == want[1] and len(want[1].splitlines()) > 0, "landmark file"
    assert python_run(orc, csv, None)[:2] != want[:2], "the run does not tell the switch off from on"
    shown = 0
    for other in ((-9.0, -4.0, -0.5), (-4.0, -0.5, -9.0), (-0.5, -9.0, -4.0)):
        if tied:
            shows = (must[0] and other[0] != HOST_CONSTS[0]) or other[1] + other[2] != HOST_CONSTS[1] + HOST_CONSTS[2]
        else:
            shows = any(must[k] and other[k] != HOST_CONSTS[k] for k in range(3))
        if shows:
            assert python_run(orc, csv, other)[:2] != want[:2], f"the run does not tell {other} from {HOST_CONSTS}"
            shown += 1
    assert shown >= 2 and (tied or shown == 3)


def test_host_program_option(orc, tmp_path):
    """slam_pf_main --assoc-weight: accepted with --assoc (with --prune and without); with 0 0 0 the pose log, the map and the
    landmark file are those of the run without it; refused without --assoc and for a constant that is none."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    angles = -2.351831 + 0.004363 * np.arange(1079)
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, 0.1, 6.0, angles=angles)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    lm, mp = tmp_path / "landmarks.csv", tmp_path / "map.csv"
    head = [str(exe), str(room), "4", "1079", str(mp), "256", "3", "--landmarks", "32"]
    det = ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)]
    assoc = ["--assoc", "9.21", "50", "--prune", "1", "1", "3", "10"]
    outs = {}
    for run, extra in (("off", []), ("zeros", ["--assoc-weight", "0", "-0", "0"]), ("on", ["--assoc-weight", "-4", "-1.5", "-0.75"])):
        r = subprocess.run(head + assoc + extra + det, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        outs[run] = (r.stdout, lm.read_bytes(), mp.read_bytes())
        assert r.stdout.count("pose =") == 3 and len(outs[run][1].splitlines()) == D.detect(rng[0], rng[1], wrap=0)[2]
    assert outs["zeros"] == outs["off"]
    r = subprocess.run(head + ["--assoc", "9.21", "50", "--assoc-weight", "-4", "-1", "-2"] + det, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr                                  # without --prune: LOG_MISS is inert
    for bad in ("1", "1e-30", "nan", "inf", "-inf", "x"):
        for slot in range(3):
            c = ["-1", "-1", "-1"]
            c[slot] = bad
            r = subprocess.run(head + assoc + ["--assoc-weight"] + c + det, capture_output=True, text=True)
            assert r.returncode == 2 and "--assoc-weight" in r.stderr, (bad, slot)
    r = subprocess.run(head + ["--assoc-weight", "-4", "-1", "-2"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
