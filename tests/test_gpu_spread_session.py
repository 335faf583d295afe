"""slam_pf_spread where it is meant to be used: a session that localises in a known landmark map, after every frame against the
restatement (tests/_spread_spec.py) applied to the poses, weights and ancestors of tests/_localise_spec.py's frame loop (the shapes
are those of tests/test_gpu_localise_session.py); slam_pf_main --spread-out against a session driven from Python through the same
frames; and the sharded form: two ranks in one process against one."""
import subprocess
import threading

import numpy as np
import pytest
import torch

import _estimate_spec as E
import _pipeline_scenes as SC
import _shard_worker as W
import _spread_spec as S
import test_gpu_localise_session as T
import test_gpu_spread as G
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
F = np.float32
rig = G.rig


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=T.L)
    x, y, th, _ = W.init_state(T.N, 0, np.zeros((0, 2), np.float32))
    M = np.zeros((5, T.L), np.float32)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::7] = -1.0
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(T.DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def _same(got, want):
    return all(np.array_equal(bits(np.asarray(g, np.float32)), bits(np.asarray(w, np.float32))) for g, w in zip(got, want[:3]))


@pytest.mark.parametrize("ess", [0.0, T.GATE_ESS], ids=["every-frame", "gated"])
def test_known_map_session_after_every_frame(world, ess):
    want = T.reference(world, world["M"], ess=ess)
    verdicts = [w["resampled"] for w in want]
    assert all(verdicts) if not ess else (True in verdicts and False in verdicts), verdicts   # gated: both forms are in play
    pkg, e, ses = T.open_session(world, ess=ess)
    ses.known_map_set(world["M"], T.GATE, T.CLUTTER)
    before = S.spread_spec(world["x"], world["y"], world["th"], None, 0.0, T.N)
    assert _same(ses.spread(0.0), before)                                  # before the first step: the plain form
    for f in range(T.FRAMES):
        e.detections_upload(*T.detections(world, f))
        ses.step(0, T.DP, True)
        w = want[f]
        w16 = None if w["resampled"] else E.weights16(w["logw"])[0]
        for ref in (0.0, 0.4):
            spec = S.spread_spec(w["pose"][0], w["pose"][1], w["pose"][2], None, ref, T.N, w16)
            got = ses.spread(ref)
            assert _same(got, spec), (f, ref, w["resampled"], [np.asarray(v).tolist() for v in got], [np.asarray(v).tolist() for v in spec[:3]])
            assert np.array_equal(bits(ses.mean(ref)), bits(spec[0]))
        T.compare(T.frame(e, ses), w, f"frame {f}")                        # asking changed nothing of the frame
    ses.close()
    e.close()


HOST_N, HOST_SEED = 4098, 3


def write_scene(path):
    """The twelve frames of tests/_pipeline_scenes.py as the program reads them: one line of 1079 ranges per frame, a sensor that moves"""
    path.write_text("".join(",".join(f"{v:.6f}" for v in np.hypot(bx.astype(np.float64), by.astype(np.float64))) + "\n" for bx, by in SC.SCANS))


def python_run(orc, csv, ess, n=None, seed=None, meas_var=1.0, configure=None, observe=False, after=None):
    """What slam_pf_main does without landmarks, from Python (the loop of tests/test_gpu_assoc_weight_session.py's python_run: the
    front end's pieces are the oracle's, pinned bit for bit on the C front end by tests/test_host_frontend.py; the session is the
    package's) -> (pose log, per frame: the frame number and what spread returned around the heading the mean was asked around, frames the gate kept).
    n, seed, meas_var: the session's (default: HOST_N, HOST_SEED, 1.0).  configure(pkg, e, ses, ang): the switches the program gives
    in front of the first frame; observe: every frame has use_observations = 1; after(ses) -> the tail of the frame's pose line
    (the program's reseed behind the frame)."""
    import ctypes
    libm = ctypes.CDLL("libm.so.6")
    libm.cosf.restype = libm.sinf.restype = ctypes.c_float
    libm.cosf.argtypes = libm.sinf.argtypes = [ctypes.c_float]
    pkg = load_package()
    frames = [np.array([float(v) for v in ln.split(",") if v.strip()], F) for ln in csv.read_text().splitlines()]
    ang = orc.beam_angles(-2.351831, 0.004363, len(frames[0]))
    e = pkg.Engine(0)
    ses = pkg.PfSession(e, n or HOST_N, 0, seed=HOST_SEED if seed is None else seed, sigma=(0.01, 0.01, 0.002), meas_var=meas_var, score_gain=0.25,
                        resample_ess_frac=ess)
    if configure:
        configure(pkg, e, ses, ang)
    pose, prev = np.zeros(3, F), np.zeros(3, F)
    bx, by = orc.clean_scan(frames[0], ang)
    map_x, map_y = orc.transform(bx, by, pose)
    map_pose = pose.copy()
    ses.reset(pose)
    updated, log, spreads, kept = True, [], [], 0
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
        ses.step(1, dp, observe)
        ref = float(F(pose[2] + dp[2]))
        kept += int(bool(ess) and not e.resample_happened())
        best = ses.mean(ref)
        got = ses.spread(ref)
        assert np.array_equal(bits(got[0]), bits(best))
        spreads.append((k + 1, got[1], got[2]))
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
        log.append("pose = %f  %f  %f%s\n" % (tuple(float(v) for v in pose) + (after(ses) if after else "",)))
    ses.close()
    e.close()
    return "".join(log), spreads, kept


def parse(path):
    """FILE -> per line (frame number, float32 [6], float32), after checking that the text is the binary32 and nothing more (%.9g)"""
    out = []
    for ln in path.read_text().splitlines():
        t = ln.split(",")
        assert len(t) == 8, ln
        v = np.array([float(u) for u in t[1:]], F)
        assert [f"{float(u):.9g}" for u in v] == t[1:], ln
        out.append((int(t[0]), v[:6], v[6]))
    return out


@pytest.mark.parametrize("dataset,ess", [("scene", 0.0), ("scene", 0.01), ("head", 0.0)])
def test_host_program_writes_what_the_session_returns(orc, tmp_path, dataset, ess):
    """slam_pf_main --spread-out on the moving-sensor scene (resampling every frame and ESS-gated with a threshold low enough that frames are
    kept: those go through the weighted form) and on the head of the recorded dataset: every line of FILE parses back to the bits Session.spread returns in a
    session driven from Python through the same frames — the frame's number, the six entries in their order, heading_r last, around
    the heading the mean was asked around — and the pose log and the map file are byte for byte those of a run without the flag."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    if dataset == "scene":
        csv = tmp_path / "scene.csv"
        write_scene(csv)
    else:
        csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[0].split(",")))]
    gate = ["--ess", f"{ess:g}"] if ess else []

    def run(tag, *extra):
        r = subprocess.run(base + [str(tmp_path / f"map_{tag}.csv"), str(HOST_N), str(HOST_SEED)] + gate + list(extra), capture_output=True,
                           text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r.stdout, (tmp_path / f"map_{tag}.csv").read_bytes()

    plain = run("plain")
    assert run("flag", "--spread-out", str(tmp_path / "spread.csv")) == plain
    got = parse(tmp_path / "spread.csv")
    log, want, kept = python_run(orc, csv, ess)
    assert (kept > 0) == bool(ess), kept                                 # gated: the weighted form was in play
    assert log == plain[0]                                               # the Python loop IS the program's
    assert [g[0] for g in got] == [w[0] for w in want] == list(range(2, len(lines) + 1))
    for g, w in zip(got, want):
        assert np.array_equal(bits(g[1]), bits(w[1])) and np.array_equal(bits(g[2]), bits(w[2])), (g, w)
    distinct = {bits(np.append(w[1], w[2])).tobytes() for w in want}
    assert len(distinct) == len(want) and all(len(set(bits(np.append(w[1], w[2])).tolist())) == 7 for w in want)   # frames and entries can be told apart


def test_host_program_two_ranks_and_a_file_it_cannot_open(orc, tmp_path):
    """Two ranks sharing the card write the single-GPU file; a FILE that cannot be opened ends the program at once, before any rank
    runs (two ranks: none is left waiting for the other)."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[0].split(","))), str(tmp_path / "map.csv"), str(HOST_N), str(HOST_SEED)]
    two = ["--gpus", "2", "--transport", "local", "--same-device"]
    for tag, extra in (("one", []), ("two", two)):
        r = subprocess.run(base + extra + ["--spread-out", str(tmp_path / f"{tag}.csv")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
    assert (tmp_path / "one.csv").read_text() == (tmp_path / "two.csv").read_text() and len(parse(tmp_path / "one.csv")) == len(lines) - 1
    r = subprocess.run(base + two + ["--spread-out", str(tmp_path / "no_such_dir" / "spread.csv")], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "no_such_dir" in r.stderr and "pose =" not in r.stdout


def _ranks(rig, world, n_total, ess, gain, frames, ref):
    """`world` ranks on this card (one host thread and one engine per rank, in-process transport; world == 1: a plain session,
    checked against the restatement) -> per rank, per frame: what spread returned"""
    pkg = rig.pkg
    n = n_total // world
    x, y, th, _ = W.init_state(n_total, 0, rig.lm[:0])
    group = pkg.LocalGroup(world) if world > 1 else None
    out, errors = [None] * world, []

    def rank_main(r):
        comm = None
        try:
            eng, keep = (rig.eng, None) if world == 1 else G._engine(pkg, rig.world)
            comm = pkg.Comm.local(eng, group, r) if group else None
            ses = G._session(rig, n, ess=ess, gain=gain, eng=eng, comm=comm)
            sl = slice(r * n, (r + 1) * n)
            ses.set_poses(x[sl], y[sl], th[sl])
            rec = [ses.spread(ref)]
            for f in range(frames):
                ses.step(0, list(E.DP))
                if world == 1:
                    G._check(eng, ses, refs=(ref,), fq=E.oracle.ess_frac_q16(ess), tag=f"one rank, frame {f}")
                rec.append(ses.spread(ref))
            out[r] = rec
            ses.close()
            if comm:
                comm.close()
            if world > 1:
                eng.close()
        except BaseException as exc:   # noqa: BLE001 - re-raised by the caller
            errors.append(exc)
            if comm:
                comm.abort()             # the other ranks fail instead of waiting

    if world == 1:
        rank_main(0)
    else:
        ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        group.close()
    if errors:
        raise errors[0]
    return out


@pytest.mark.parametrize("ess,gain", [(0.0, 1.0), (0.5, 0.1)])
def test_two_ranks_equal_one_rank(rig, ess, gain):
    """n_total = 8 194 as two ranks of 4 097 sharing this card against one rank, before the first step and after every frame: both
    ranks return the single-GPU bits (which are the restatement's, checked inside)."""
    n_total, frames = 2 * 4097, 4
    one = _ranks(rig, 1, n_total, ess, gain, frames, 0.07)[0]
    two = _ranks(rig, 2, n_total, ess, gain, frames, 0.07)
    for f in range(frames + 1):
        for r in range(2):
            assert G._same(two[r][f], one[f]), (f, r, G._show(two[r][f]), G._show(one[f]))
