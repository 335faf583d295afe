"""A rows session with the detector on (slam_pf_assoc_set + slam_pf_detect_set, with and without slam_pf_prune_set and
slam_pf_refine_set, ESS-gated and not) against the frame loop of tests/_detect_spec.py over frames with a different scan each:
poses, maps, association tables, evidence and stats bit for bit; the refusals; switching the detector off and handing the same
detections over by hand gives the same bits; and slam_pf_main grows a landmark map from nothing but lidar frames."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_spec as D
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS, L, FRAMES = (4, 257), 64, 6
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 3, 4.0)
GATE_ESS = 0.5
REFINE = (0.05, 0.008727, 1)
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]
RHO, HALF = 0.1, 5.0
POLES = np.random.default_rng(12).uniform(-4.0, 4.0, (12, 2))


def scan(f):
    """Frame f: the pole room as the moving sensor sees it, 360 beams with 1 cm of range noise — another scan every frame."""
    pose = (f + 1) * np.array(DP)
    bx, by, _, _ = D.raycast(pose, POLES, RHO, HALF, 360, noise=np.random.default_rng(900 + f))
    return bx, by


SCANS = [scan(f) for f in range(FRAMES)]


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, _, _, _ = W.make_world(L=L)
    x, y, th, _ = W.init_state(max(NS), 0, np.zeros((0, 2), np.float32))
    mp = np.zeros((max(NS), 5, L), np.float32)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), x=x, y=y, th=th, mp=mp)


def open_session(world, n, ess=0.0, layout="rows", assoc=True, prune=None, refine=None):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    ses = pkg.PfSession(e, n, L, resample_ess_frac=ess, map_layout=layout, **KW)
    if refine:
        ses.refine_set(*refine)
    if assoc:
        ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"][:n], world["y"][:n], world["th"][:n])
    ses.set_map(world["mp"][:n])
    if prune:
        ses.prune_set(*prune)
    return e, ses


def frame(e, ses, n, prune):
    v = ses.device_view()
    av = ses.assoc_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy(),
              assoc=torch.as_tensor(av["assoc"], device=DEV).cpu().numpy(), stats=torch.as_tensor(av["stats"], device=DEV).cpu().numpy())
    if prune:
        ev = ses.evidence_view()
        fr["ev"] = ses.evidence()
        fr["ev_stats"] = torch.as_tensor(ev["stats"], device=DEV).cpu().numpy()
    return fr


def compare(g, w, label, prune):
    assert np.array_equal(g["assoc"][:, :L], w["assoc"][:, :L]) and np.all(g["assoc"][:, L:] == 255), f"{label}: association table"
    assert np.array_equal(g["stats"], w["stats"]), f"{label}: association stats"
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    if prune:
        assert np.array_equal(g["ev"], w["ev"]), f"{label}: evidence"
        assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"{label}: evidence stats"


@pytest.mark.parametrize("refine", [None, REFINE], ids=["plain", "refined"])
@pytest.mark.parametrize("prune", [None, PRUNE], ids=["assoc", "pruning"])
@pytest.mark.parametrize("ess", [0.0, GATE_ESS], ids=["every-frame", "gated"])
@pytest.mark.parametrize("n", NS)
def test_session_equals_the_spec_loop(world, n, ess, prune, refine):
    want = D.frame_loop(world, SCANS, n, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=prune, ess=ess, refine=refine, **KW)
    ndet = [len(w["det"][0]) for w in want]
    assert min(ndet) >= 3 and len(set(bits(w["det"][0]).tobytes() for w in want)) == FRAMES        # detections, others every frame
    assert sum(int(w["stats"][:, 1].sum()) for w in want) > 0 and int(want[-1]["stats"][:, 0].sum()) > 0   # landmarks made, then matched
    e, ses = open_session(world, n, ess=ess, prune=prune, refine=refine)
    ses.detect_set()
    c0, a0, v0 = e.detect_count(), e.assoc_counts(), e.evidence_counts()
    for f in range(FRAMES):
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, n, prune), want[f], f"n={n} frame {f}", prune)
        zx, zy = e.detections()
        assert np.array_equal(bits(zx), bits(want[f]["det"][0])) and np.array_equal(bits(zy), bits(want[f]["det"][1]))
    assert e.detect_count() - c0 == FRAMES and tuple(np.subtract(e.assoc_counts(), a0)) == (FRAMES, FRAMES)
    assert tuple(np.subtract(e.evidence_counts(), v0)) == ((FRAMES, 0) if prune else (0, 0))
    # a frame without observations launches no detector
    ses.step(0, DP, False)
    assert e.detect_count() - c0 == FRAMES
    ses.close()
    e.close()


def test_switched_off_and_fed_by_hand_gives_the_same_bits(world):
    """Frames 0-2 with the detector, 3-5 with it off and the spec's detections uploaded; and slam_pf_assoc_set(0) takes it off."""
    n = NS[1]
    want = D.frame_loop(world, SCANS, n, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, **KW)
    e, ses = open_session(world, n, prune=PRUNE)
    ses.detect_set(load_package().DetectParams.default())
    for f in range(FRAMES):
        e.scan_upload(*SCANS[f])
        if f == 3:
            ses.detect_set(None)
            c3 = e.detect_count()
        if f >= 3:
            e.detections_upload(*want[f]["det"])
        ses.step(0, DP, True)
        compare(frame(e, ses, n, PRUNE), want[f], f"frame {f}", PRUNE)
    assert e.detect_count() == c3
    ses.detect_set()
    ses.assoc_set(0.0)                           # association off: the detector goes with it, and stays off
    ses.assoc_set(GATE, NEW_GATE, True)
    e.detections_upload(*want[0]["det"])
    ses.step(0, DP, True)
    assert e.detect_count() == c3
    ses.close()
    e.close()


@pytest.mark.parametrize("case", ["association off", "split", "bad parameters"])
def test_refusals(world, case):
    """... and the session then steps exactly as one that was never asked."""
    pkg = load_package()
    n = NS[1]
    ids = np.arange(5, dtype=np.int32)
    z = np.linspace(-2, 2, 5).astype(np.float32)
    out = []
    for ask in (False, True):
        e, ses = open_session(world, n, layout="split" if case == "split" else "rows", assoc=case == "bad parameters")
        if ask:
            if case == "split":
                with pytest.raises(pkg.SlamError):
                    ses.assoc_set(GATE, NEW_GATE, True)
            with pytest.raises(pkg.SlamError) as err:
                ses.detect_set(min_points=0) if case == "bad parameters" else ses.detect_set()
            assert err.value.status == -2
            assert ("data association" if case != "bad parameters" else "min_points") in str(err.value), str(err.value)
        frames = []
        for f in range(2):
            e.scan_upload(*SCANS[f])
            e.obs_upload(ids, z, z[::-1].copy(), L)
            e.detections_upload(z, z)
            ses.step(0, DP, True)
            frames.append((ses.poses(), ses.maps()))
        assert e.detect_count() == 0
        out.append(frames)
        ses.close()
        e.close()
    for f in range(2):
        for g, w in zip(out[1][f], out[0][f]):
            assert np.array_equal(bits(g), bits(w)), f"{case}: frame {f}"


def test_host_program_grows_a_landmark_map(orc, tmp_path):
    """slam_pf_main --landmarks 32 --assoc ... --detect --landmarks-out on the head of the recorded dataset; and without
    --landmarks the new binary's outputs are those of a run without any of the new options."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    lm = tmp_path / "landmarks.csv"
    r = subprocess.run(base + [str(tmp_path / "map_lm.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50", "--prune", "1", "1",
                               "3", "10", "--detect", "--landmarks-out", str(lm)], capture_output=True, text=True)
    print(r.stderr.strip())
    assert r.returncode == 0, r.stderr
    rows = lm.read_text().splitlines()
    assert len(rows) <= 32
    for ln in rows:
        vals = [float(v) for v in ln.split(",")]
        assert len(vals) == 2 and np.isfinite(vals).all()
    # explicit parameters (a 270-degree sensor: no wrap), and the pose log is still there
    r = subprocess.run(base + [str(tmp_path / "map_lm2.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50", "--detect", "0.3",
                               "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("pose =") == len(lines) - 1, r.stderr
    assert len(lm.read_text().splitlines()) <= 32
    # without --landmarks: the run of a program that has none of the new options (its landmark-free session, frame for frame)
    runs = []
    for k in range(2):
        r = subprocess.run(base + [str(tmp_path / f"map{k}.csv"), "256", "3"] + (["--ess", "0.5"] if k else []), check=True,
                           capture_output=True, text=True)
        runs.append((r.stdout, (tmp_path / f"map{k}.csv").read_bytes()))
        assert r.stdout.count("pose =") == len(lines) - 1
    r = subprocess.run(base + [str(tmp_path / "map2.csv"), "256", "3"], check=True, capture_output=True, text=True)
    assert (r.stdout, (tmp_path / "map2.csv").read_bytes()) == runs[0]
    # a scene that HAS poles, seen by the program's own sensor (1079 beams over 270 degrees: no wrap) from the origin, four times:
    # the map file holds landmarks, each at a pole — the centroid lies within RHO of the centre, the filter's poses within
    # centimetres of the origin after three frames of 1 cm motion noise
    # (the poles on a ring, 30 degrees apart: no narrow piece of wall shows between two of them — the rule would take it for a pole)
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    ang = -2.351831 + 0.004363 * np.arange(1079)
    rng = D.raycast((0.0, 0.0, 0.0), poles, RHO, 6.0, angles=ang)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    r = subprocess.run([str(exe), str(room), "4", "1079", str(tmp_path / "map_room.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21",
                        "50", "--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)], capture_output=True, text=True)
    print(r.stderr.strip())
    assert r.returncode == 0, r.stderr
    zx, zy, k, _ = D.detect(rng[0], rng[1], wrap=0)
    found = np.array([[float(v) for v in ln.split(",")] for ln in lm.read_text().splitlines()])
    assert k >= 3 and len(found) == k
    d = np.hypot(found[:, None, 0] - poles[None, :, 0], found[:, None, 1] - poles[None, :, 1]).min(axis=1)
    assert np.all(d <= RHO + 0.1), d
    # the landmark options without --landmarks are refused with the usage text
    r = subprocess.run(base + [str(tmp_path / "map3.csv"), "256", "3", "--detect"], capture_output=True, text=True)
    assert r.returncode == 2 and "--landmarks" in r.stderr
