"""A rows session with association, pruning, the detector (wrap = 0) and the field of view (slam_pf_prune_fov_set), with line of
sight and without, against the frame loop of tests/_fov_spec.py over the forty frames of the drive of test_fov_behaviour_cpu.py —
the reference's 269.5-degree sensor past a pole that drifts into the blind quarter: poses, maps, evidence, stats, spared and
outside counts bit for bit; with on = 0 the session is today's, launch for launch; the refusals; and slam_pf_main --prune-fov."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_spec as D
import _fov_spec as V
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
N, L, FRAMES = 64, 8, 40
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 8, 9.0)
SIGHT = (128, 0.3)
EDGE = 0.1
KW = dict(seed=5, sigma=(0.005, 0.005, 0.001), meas_var=2.5e-3, score_gain=0.05)
DP = [0.0, 0.03, 0.0]
RHO, HALF = 0.1, 6.0
ANGLES = -2.351831 + 0.004363 * np.arange(1079)
POLES = np.array([(-1.5, 2), (3, -2), (4, .6), (1, 3.5), (2.5, 3)], np.float64)
SCANS = [D.raycast((0.0, 0.03 * (f + 1), 0.0), POLES, RHO, HALF, noise=np.random.default_rng(100 + f), angles=ANGLES)[:2] for f in range(FRAMES)]
ARC = (float(F(ANGLES[0])), float(F(ANGLES[-1])), EDGE)


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, _, _, _ = W.make_world(L=L)
    mp = np.zeros((N, 5, L), F)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), x=np.zeros(N, F), y=np.zeros(N, F), th=np.zeros(N, F), mp=mp)


def spec(world, fov, sight, frames=FRAMES):
    return V.frame_loop(world, SCANS[:frames], N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, fov=fov, sight=sight,
                        detect_params=dict(wrap=0), **KW)


def open_session(world, fov=None, sight=None):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    ses = pkg.PfSession(e, N, L, map_layout="rows", **KW)
    ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    ses.prune_set(*PRUNE)
    ses.detect_set(wrap=0)
    if sight:
        ses.prune_sight_set(*sight)
    if fov:
        ses.prune_fov_set(True, *fov)
    return e, ses


def frame(e, ses, fov, sight):
    v, ev = ses.device_view(), ses.evidence_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy(), ev=ses.evidence(),
              ev_stats=torch.as_tensor(ev["stats"], device=DEV).cpu().numpy())
    if fov:
        fr["outside"] = torch.as_tensor(ses.fov_view()["outside"], device=DEV).cpu().numpy()
    if sight:
        fr["spared"] = torch.as_tensor(ses.sight_view()["spared"], device=DEV).cpu().numpy()
    return fr


def compare(g, w, label):
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    assert np.array_equal(g["ev"], w["ev"]), f"{label}: evidence"
    assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"{label}: evidence stats"
    for k in ("outside", "spared"):
        if k in g:
            assert np.array_equal(g[k], w[k]), f"{label}: {k}"


@pytest.mark.parametrize("sight", [None, SIGHT], ids=["plain", "sight"])
def test_session_equals_the_spec_loop(world, sight):
    e, ses = open_session(world, ARC, sight)
    lo, hi = ses.fov_view()["bounds"]            # the bounds the library's cosine and sine gave: the spec's from here on
    want_lo, want_hi = V.bound(F(ARC[0]) + F(EDGE)), V.bound(F(ARC[1]) - F(EDGE))
    assert lo > hi and abs(lo - want_lo) < 1e-6 and abs(hi - want_hi) < 1e-6
    want, off = spec(world, (lo, hi), sight), spec(world, None, sight)
    # what the frames hold: landmarks outside the arc in the later frames, and a rule that changes the outcome
    outside = [int(w["outside"].sum()) for w in want]
    prunes = [sum(int(w["ev_stats"][:, 0].sum()) for w in run) for run in (off, want)]
    assert sum(outside[20:]) > 0 and prunes[0] > prunes[1]
    c0, s0, v0 = e.fov_counts(), e.sight_counts(), e.evidence_counts()
    for f in range(FRAMES):
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, True, sight), want[f], f"frame {f}")
    # one stage per observing frame in its own counter, one table per frame with line of sight, and not one launch of the stages it replaces
    assert e.fov_counts() == c0 + FRAMES and e.evidence_counts() == v0
    assert e.sight_counts() == (s0[0] + (FRAMES if sight else 0), s0[1])
    ses.step(0, DP, False)                       # a frame without observations runs no stage
    assert e.fov_counts() == c0 + FRAMES
    ses.prune_set(0)                             # pruning off: the field of view is not in force
    e.scan_upload(*SCANS[0])
    ses.step(0, DP, True)
    assert e.fov_counts() == c0 + FRAMES and e.evidence_counts() == v0
    ses.close()
    e.close()


@pytest.mark.parametrize("sight", [None, SIGHT], ids=["plain", "sight"])
def test_on_zero_is_todays_session(world, sight):
    frames = 12
    want = spec(world, None, sight, frames)
    runs, counts = [], []
    for ask in (False, True):
        e, ses = open_session(world, None, sight)
        if ask:
            ses.prune_fov_set(True, *ARC)
            ses.prune_fov_set(False)
            assert tuple(float(b) for b in ses.fov_view()["bounds"]) == (0.0, 4.0)
        got = []
        for f in range(frames):
            e.scan_upload(*SCANS[f])
            ses.step(0, DP, True)
            got.append(frame(e, ses, False, sight))
            compare(got[-1], want[f], f"frame {f}")
        counts.append((e.fov_counts(), e.sight_counts(), e.evidence_counts(), e.assoc_counts(), e.detect_count()))
        assert counts[-1][0] == 0
        runs.append(got)
        ses.close()
        e.close()
    assert counts[0] == counts[1]
    for f in range(frames):
        for k in runs[0][f]:
            assert runs[0][f][k].tobytes() == runs[1][f][k].tobytes(), (f, k)


def test_refusals(world):
    pkg = load_package()
    e, ses = open_session(world)
    with pytest.raises(pkg.SlamError) as err:
        ses.fov_view()                           # never switched on
    assert err.value.status == -4
    nan, inf, pi = float("nan"), float("inf"), float(F(np.pi))
    above = float(np.nextafter(F(np.pi), F(4)))
    for bad in ((nan, 2.0, 0.1), (-2.0, nan, 0.1), (-2.0, 2.0, nan), (-inf, 2.0, 0.1), (-2.0, inf, 0.1), (-2.0, 2.0, inf), (-2.0, 2.0, -0.1),
                (-above, 2.0, 0.0), (-2.0, above, 0.0), (-2.0, 2.0, 2.0), (1.0, 1.0, 0.0), (2.0, -2.0, 0.0), (-1.0, 1.0, 1.0)):
        with pytest.raises(pkg.SlamError) as err:
            ses.prune_fov_set(True, *bad)
        assert err.value.status == -2 and "field of view" in str(err.value), bad
    with pytest.raises(pkg.SlamError):
        ses.fov_view()                           # a refused call switched nothing on
    ses.prune_fov_set(True, -pi, pi, 0.0)        # the whole circle is an arc
    ses.assoc_set(0.0)                           # association off: refused as slam_pf_prune_sight_set is
    with pytest.raises(pkg.SlamError) as err:
        ses.prune_fov_set(True, *ARC)
    assert err.value.status == -2 and "data association" in str(err.value)
    ses.prune_fov_set(False)                     # off is always accepted
    ses.assoc_set(GATE, NEW_GATE, True)
    ses.prune_fov_set(True, *ARC)
    lo, hi = ses.fov_view()["bounds"]
    assert lo == pkg.fov_bound(float(F(ARC[0]) + F(EDGE))) and hi == pkg.fov_bound(float(F(ARC[1]) - F(EDGE)))
    ses.assoc_set(0.0)                           # ... and association off takes it off
    ses.assoc_set(GATE, NEW_GATE, True)
    assert tuple(float(b) for b in ses.fov_view()["bounds"]) == (0.0, 4.0)
    ses.close()
    e.close()


def test_host_program_option(orc, tmp_path):
    """slam_pf_main --prune-fov: accepted with --prune (with --prune-sight and without); an edge that leaves no arc is refused by
    slam_pf_prune_fov_set."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, RHO, 6.0, angles=ANGLES)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    lm = tmp_path / "landmarks.csv"
    base = [str(exe), str(room), "4", "1079", str(tmp_path / "map.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50",
            "--prune", "1", "1", "3", "10"]
    det = ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)]
    k = D.detect(rng[0], rng[1], wrap=0)[2]
    for extra in ([], ["--prune-sight", "128", "0.3"]):
        r = subprocess.run(base + extra + ["--prune-fov", "0.1"] + det, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        assert k >= 3 and len(lm.read_text().splitlines()) == k
    r = subprocess.run(base + ["--prune-fov", "2.5"] + det, capture_output=True, text=True)
    assert r.returncode != 0 and "slam_pf_prune_fov_set" in r.stderr
