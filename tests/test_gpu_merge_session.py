"""A rows session with data association and merging (slam_pf_merge_set) against the frame loop of tests/_merge_spec.py over twelve
frames, bit for bit: poses, map rows, evidence, log-weights, ancestors and merge stats — with pruning, under a 2x2 measurement
covariance, and with a resample gate (frames that keep their population run the stage in place); with the switch off the session
is today's, launch for launch; the refusals; and slam_pf_main --merge end to end.

The detections: the true points, and in every frame a second, displaced return of one of them — beyond the association's gates, so
it starts a duplicate landmark that no later frame confirms: the next frame's stage merges it into the landmark of its pole."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_spec as D
import _merge_spec as M
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 300, 40, 12
GATE, NEW_GATE, MERGE_GATE = 9.21, 9.21, 40.0
PRUNE = (1, 1, 4, 3.5)
COV = (0.03, 0.008, 0.015)
GATE_ESS = 0.5
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]
TRUE = np.random.default_rng(3).uniform(-3, 3, (7, 2)).astype(np.float32)
SETUPS = {"pruning": dict(prune=PRUNE), "2x2 Q": dict(meas_cov=COV), "resample gate": dict(prune=PRUNE, ess=GATE_ESS)}


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, _ = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    mp = np.zeros((N, 5, L), np.float32)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, x=x, y=y, th=th, mp=mp)


def detections(f):
    rng = np.random.default_rng(900 + f)
    keep = rng.random(len(TRUE)) >= 0.2
    keep[f % len(TRUE)] = True
    seen = TRUE - np.float32(f + 1) * np.array(DP[:2], np.float32)
    z = seen[keep] + 0.02 * rng.standard_normal((int(keep.sum()), 2)).astype(np.float32)
    a = rng.uniform(0, 2 * np.pi)
    ghost = seen[f % len(TRUE)] + 0.7 * np.array([np.cos(a), np.sin(a)], np.float32)   # the displaced second return
    z = np.concatenate([z, ghost[None]])
    z = z[rng.permutation(len(z))].astype(np.float32)
    return z[:, 0].copy(), z[:, 1].copy()


def reference(world, merge_gate=MERGE_GATE, frames=FRAMES, prune=None, meas_cov=None, ess=0.0):
    return M.frame_loop(world, N, frames, dp=DP, detections=detections, gate=GATE, new_gate=NEW_GATE, create=1, merge_gate=merge_gate,
                        meas_cov=meas_cov, prune=prune, ess=ess, **KW)


def open_session(world, prune=None, meas_cov=None, ess=0.0, layout="rows", comm_group=None, assoc=True):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    if assoc and meas_cov:
        ses.assoc_cov_set(meas_cov, GATE, NEW_GATE, True)
    elif assoc:
        ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    if prune:
        ses.prune_set(*prune)
    return e, ses, comm


def close_session(e, ses, comm=None):
    ses.close()
    if comm:
        comm.close()
    e.close()


def step(e, ses, f, prune, merging=True):
    e.detections_upload(*detections(f))
    ses.step(0, DP, True)
    v = ses.device_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy())
    if prune:
        fr["ev"] = ses.evidence()
        fr["ev_stats"] = torch.as_tensor(ses.evidence_view()["stats"], device=DEV).cpu().numpy()
    if merging:
        fr["merge_stats"] = torch.as_tensor(ses.merge_view(), device=DEV).cpu().numpy()
    return fr


def compare(g, w, label):
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    for k in ("ev", "ev_stats", "merge_stats"):
        if k in g:
            assert np.array_equal(g[k], w[k]), f"{label}: {k}"


@pytest.mark.parametrize("setup", list(SETUPS))
def test_session_equals_the_spec_loop(world, setup):
    kw = SETUPS[setup]
    want, off = reference(world, **kw), reference(world, merge_gate=0.0, **kw)
    merged = sum(int(w["merge_stats"][:, 0].sum()) for w in want)
    seen = [int((~(run[-1]["map"][:, 2] < 0)).sum()) for run in (off, want)]
    assert merged > N and seen[1] < seen[0], (merged, seen)      # the frames hold merges, and the maps end smaller for them
    if kw.get("ess"):
        kept = [not w["resampled"] for w in want]
        assert any(kept) and not all(kept)                         # frames in place and frames through the gather
    e, ses, _ = open_session(world, **kw)
    ses.merge_set(MERGE_GATE)
    c0, a0, v0 = e.merge_count(), e.assoc_counts(), e.evidence_counts()
    for f in range(FRAMES):
        compare(step(e, ses, f, kw.get("prune")), want[f], f"{setup}: frame {f}")
    # one stage per observing frame in its own counter, and the other stages as they were
    assert e.merge_count() == c0 + FRAMES
    if not kw.get("meas_cov"):                                     # (the stages under a 2x2 Q count elsewhere)
        assert tuple(np.subtract(e.assoc_counts(), a0)) == (FRAMES, FRAMES)
    assert tuple(np.subtract(e.evidence_counts(), v0)) == ((FRAMES, 0) if kw.get("prune") else (0, 0))
    ses.step(0, DP, False)                                         # a frame without observations runs no stage
    assert e.merge_count() == c0 + FRAMES
    close_session(e, ses)


def test_switched_off_is_todays_session(world):
    frames = 6
    want = reference(world, merge_gate=0.0, frames=frames, prune=PRUNE)
    runs, counts = [], []
    for ask in (False, True):
        e, ses, _ = open_session(world, prune=PRUNE)
        if ask:
            ses.merge_set(MERGE_GATE)
            ses.merge_set(0.0)
        got = []
        for f in range(frames):
            got.append(step(e, ses, f, PRUNE, merging=False))
            compare(got[-1], want[f], f"frame {f}")
        counts.append((e.merge_count(), e.evidence_counts(), e.assoc_counts()))
        assert counts[-1][0] == 0
        runs.append(got)
        close_session(e, ses)
    assert counts[0] == counts[1]
    for f in range(frames):
        for k in runs[0][f]:
            assert runs[0][f][k].tobytes() == runs[1][f][k].tobytes(), (f, k)


def test_switches_and_bad_gates(world):
    pkg = load_package()
    e, ses, _ = open_session(world)
    with pytest.raises(pkg.SlamError) as err:
        ses.merge_view()                                           # never switched on
    assert err.value.status == -4
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(pkg.SlamError) as err:
            ses.merge_set(bad)
        assert err.value.status == -2 and "merge_gate" in str(err.value), bad
    with pytest.raises(pkg.SlamError):
        ses.merge_view()                                           # a refused call switched nothing on
    ses.merge_set(MERGE_GATE)
    ses.assoc_set(0.0)                                             # association off takes merging off ...
    with pytest.raises(pkg.SlamError) as err:
        ses.merge_set(MERGE_GATE)                                  # ... and it is refused while association is off
    assert err.value.status == -2 and "data association" in str(err.value)
    ses.merge_set(0.0)                                             # off is always accepted
    ses.assoc_detcov_set(GATE, NEW_GATE, True)                     # accepted under each of the noise forms
    ses.merge_set(MERGE_GATE)
    ses.assoc_cov_set(COV, GATE, NEW_GATE, True)
    ses.merge_set(MERGE_GATE)
    ses.assoc_set(GATE, NEW_GATE, True)
    c0 = e.merge_count()
    step(e, ses, 0, None)
    assert e.merge_count() == c0 + 1                               # still on across the change of noise form
    close_session(e, ses)


@pytest.mark.parametrize("case", ["association off", "split", "pages", "auto", "sharded"])
def test_refusals(world, case):
    """... and the session then steps exactly as one that was never asked."""
    pkg = load_package()
    group = pkg.LocalGroup(1) if case == "sharded" else None
    layout = case if case in ("split", "pages", "auto") else "rows"
    ids = np.arange(5, dtype=np.int32)
    out = []
    for ask in (False, True):
        e, ses, comm = open_session(world, layout=layout, comm_group=group if ask else None, assoc=False)
        if ask:
            if case != "association off":
                with pytest.raises(pkg.SlamError):
                    ses.assoc_set(GATE, NEW_GATE, True)
            with pytest.raises(pkg.SlamError) as err:
                ses.merge_set(MERGE_GATE)
            assert err.value.status == -2 and "data association" in str(err.value), str(err.value)
            with pytest.raises(pkg.SlamError) as err:
                ses.merge_view()
            assert err.value.status == -4
        frames = []
        for f in range(2):
            e.obs_upload(ids, TRUE[:5, 0].copy(), TRUE[:5, 1].copy(), L)
            ses.step(0, DP, True)
            frames.append((ses.poses(), ses.maps()))
        assert e.merge_count() == 0
        out.append(frames)
        close_session(e, ses, comm)
    if group:
        group.close()
    for f in range(2):
        for g, w in zip(out[1][f], out[0][f]):
            assert np.array_equal(bits(g), bits(w)), f"{case}: frame {f}"


def test_host_program_option(orc, tmp_path):
    """slam_pf_main --merge: accepted with --assoc (with --prune and without); refused without --assoc and for a gate that is none."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    angles = -2.351831 + 0.004363 * np.arange(1079)
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, 0.1, 6.0, angles=angles)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    lm = tmp_path / "landmarks.csv"
    head = [str(exe), str(room), "4", "1079", str(tmp_path / "map.csv"), "256", "3", "--landmarks", "32"]
    det = ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)]
    k = D.detect(rng[0], rng[1], wrap=0)[2]
    for extra in ([], ["--prune", "1", "1", "3", "10"]):
        r = subprocess.run(head + ["--assoc", "9.21", "50", "--merge", "9.21"] + extra + det, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert k >= 3 and len(lm.read_text().splitlines()) == k   # a standing sensor: one landmark per pole, nothing to merge
    for bad in ("0", "-1", "nan", "inf", "x"):
        r = subprocess.run(head + ["--assoc", "9.21", "50", "--merge", bad] + det, capture_output=True, text=True)
        assert r.returncode == 2 and "--merge" in r.stderr, bad
    r = subprocess.run(head + ["--merge", "9.21"], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
