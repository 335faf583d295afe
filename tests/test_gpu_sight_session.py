"""A rows session with association, pruning, the detector and line of sight (slam_pf_prune_sight_set) against the frame loop of
tests/_sight_spec.py over twelve frames of the drive of test_sight_behaviour_cpu.py — the stretch in which pole 1 comes to stand in
front of pole 0: poses, maps, evidence, stats and spared counts bit for bit; with bins = 0 the session is today's, launch for
launch; the counters; switching line of sight on in mid-run; the refusals; and slam_pf_main --prune-sight."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_spec as D
import _shard_worker as W
import _sight_spec as S
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES, FIRST = 64, 8, 12, 6             # drive frames 6 .. 17: pole 0 gives detections up to frame 9, none from 10 on
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 8, 9.0)
SIGHT = (128, 0.3)
KW = dict(seed=5, sigma=(0.005, 0.005, 0.001), meas_var=2.5e-3, score_gain=0.05)
DP = [0.0, 0.03, 0.0]
RHO, HALF = 0.1, 6.0
POLES = np.array([(4, .6), (2, .6), (3, -2), (-3, 1), (1, 3.5), (-2, -3)], np.float64)
SCANS = [D.raycast((0.0, 0.03 * (FIRST + f + 1), 0.0), POLES, RHO, HALF, 360, noise=np.random.default_rng(100 + FIRST + f))[:2]
         for f in range(FRAMES)]


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, _, _, _ = W.make_world(L=L)
    mp = np.zeros((N, 5, L), np.float32)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), x=np.zeros(N, np.float32),
                y=np.full(N, 0.03 * FIRST, np.float32), th=np.zeros(N, np.float32), mp=mp)


def spec(world, sight):
    return S.frame_loop(world, SCANS, N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, sight=sight, **KW)


@pytest.fixture(scope="module")
def want_sight(world):
    return spec(world, SIGHT)


def open_session(world, sight=None):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    ses = pkg.PfSession(e, N, L, map_layout="rows", **KW)
    ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    ses.prune_set(*PRUNE)
    ses.detect_set()
    if sight:
        ses.prune_sight_set(*sight)
    return e, ses


def frame(e, ses, sight):
    v, ev = ses.device_view(), ses.evidence_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy(), ev=ses.evidence(),
              ev_stats=torch.as_tensor(ev["stats"], device=DEV).cpu().numpy())
    if sight:
        sv = ses.sight_view()
        fr["spared"] = torch.as_tensor(sv["spared"], device=DEV).cpu().numpy()
        fr["table"] = torch.as_tensor(sv["table"], device=DEV).cpu().numpy()[:sv["bins"]]
    return fr


def compare(g, w, label, sight=True):
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    assert np.array_equal(g["ev"], w["ev"]), f"{label}: evidence"
    assert np.array_equal(g["ev_stats"], w["ev_stats"]), f"{label}: evidence stats"
    if sight:
        assert np.array_equal(bits(g["table"]), bits(w["table"])), f"{label}: sight table"
        assert np.array_equal(g["spared"], w["spared"]), f"{label}: spared"


def test_session_equals_the_spec_loop(world, want_sight):
    want, plain = want_sight, spec(world, None)
    spared = [int(w["spared"].sum()) for w in want]
    # what the frames hold: landmarks spared a miss in the later frames, and a rule that changes the outcome — without it the
    # hidden pole's landmark is pruned in these frames, with it nothing is
    prunes = [sum(int(w["ev_stats"][:, 0].sum()) for w in run) for run in (plain, want)]
    assert sum(spared) > 0 and prunes[0] > prunes[1]
    assert any(not np.array_equal(a["ev"], b["ev"]) for a, b in zip(want, plain))
    e, ses = open_session(world, SIGHT)
    s0, v0 = e.sight_counts(), e.evidence_counts()
    for f in range(FRAMES):
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, True), want[f], f"frame {f}")
    # one table and one stage per observing frame, and not one launch of the stage they replace
    assert tuple(np.subtract(e.sight_counts(), s0)) == (FRAMES, FRAMES) and e.evidence_counts() == v0
    ses.step(0, DP, False)                       # a frame without observations builds no table
    assert tuple(np.subtract(e.sight_counts(), s0)) == (FRAMES, FRAMES)
    ses.close()
    e.close()


def test_bins_zero_is_todays_session(world):
    want = D.frame_loop(world, SCANS[:6], N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, **KW)
    runs = []
    for ask in (False, True):
        e, ses = open_session(world)
        if ask:
            ses.prune_sight_set(*SIGHT)
            ses.prune_sight_set(0, 0.0)
        frames = []
        for f in range(6):
            e.scan_upload(*SCANS[f])
            ses.step(0, DP, True)
            frames.append(frame(e, ses, False))
            compare(frames[-1], want[f], f"frame {f}", sight=False)
        assert e.sight_counts() == (0, 0) and e.evidence_counts()[0] == 6
        runs.append(frames)
        ses.close()
        e.close()
    for f in range(6):
        for k in runs[0][f]:
            assert runs[0][f][k].tobytes() == runs[1][f][k].tobytes(), (f, k)


def test_switched_on_in_mid_run(world):
    want = spec(world, lambda f: SIGHT if f >= 6 else None)
    assert sum(int(w["spared"].sum()) for w in want[6:]) > 0
    e, ses = open_session(world)
    for f in range(FRAMES):
        if f == 6:
            ses.prune_sight_set(*SIGHT)
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, f >= 6), want[f], f"frame {f}", sight=f >= 6)
    assert e.sight_counts() == (6, 6) and e.evidence_counts()[0] == 6
    ses.prune_set(0)                             # pruning off: line of sight is not in force, and comes back with it
    e.scan_upload(*SCANS[0])
    ses.step(0, DP, True)
    assert e.sight_counts() == (6, 6) and e.evidence_counts()[0] == 6
    ses.close()
    e.close()


def test_refusals(world):
    pkg = load_package()
    e, ses = open_session(world)
    with pytest.raises(pkg.SlamError) as err:
        ses.sight_view()                         # never switched on
    assert err.value.status == -4
    for bins, margin in ((16, 0.3), (96, 0.3), (2048, 0.3), (128, 0.0), (128, -1.0), (128, float("nan")), (128, float("inf"))):
        with pytest.raises(pkg.SlamError) as err:
            ses.prune_sight_set(bins, margin)
        assert err.value.status == -2 and "bins" in str(err.value), (bins, margin)
    ses.assoc_set(0.0)                           # association off: refused as slam_pf_prune_set is
    with pytest.raises(pkg.SlamError) as err:
        ses.prune_sight_set(*SIGHT)
    assert err.value.status == -2 and "data association" in str(err.value)
    ses.assoc_set(GATE, NEW_GATE, True)
    ses.prune_sight_set(*SIGHT)
    assert ses.sight_view()["bins"] == 128
    ses.assoc_set(0.0)                           # ... and association off takes it off
    ses.assoc_set(GATE, NEW_GATE, True)
    assert ses.sight_view()["bins"] == 0
    ses.close()
    e.close()


def test_host_program_option(orc, tmp_path):
    """slam_pf_main --prune-sight: accepted with --prune, an error without it (before any engine call)."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    ang = -2.351831 + 0.004363 * np.arange(1079)
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    rng = D.raycast((0.0, 0.0, 0.0), poles, RHO, 6.0, angles=ang)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    lm = tmp_path / "landmarks.csv"
    base = [str(exe), str(room), "4", "1079", str(tmp_path / "map.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50"]
    det = ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0", "--landmarks-out", str(lm)]
    r = subprocess.run(base + ["--prune", "1", "1", "3", "10", "--prune-sight", "128", "0.3"] + det, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    k = D.detect(rng[0], rng[1], wrap=0)[2]
    assert k >= 3 and len(lm.read_text().splitlines()) == k
    r = subprocess.run(base + ["--prune-sight", "128", "0.3"] + det, capture_output=True, text=True)
    assert r.returncode == 2 and "--prune-sight" in r.stderr
    r = subprocess.run(base + ["--prune", "1", "1", "3", "10", "--prune-sight", "100", "0.3"] + det, capture_output=True, text=True)
    assert r.returncode != 0                     # bins that are no power of two: slam_pf_prune_sight_set refuses
