"""A session that localises in a known map AND charges the landmarks in view that no detection matched
(slam_pf_known_map_miss_set) against the frame loop of tests/_localise_miss_spec.py, frame by frame and bit for bit through the
device views: poses, log-weights, ancestors, stats and the three counts — both noise forms, with uploaded detections and with the
detector, resampling every frame and ESS-gated; the mode switched on and off between frames; the launch counters with the mode
off; every refusal; and slam_pf_main --known-miss."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_noise_spec as DN
import _detect_spec as D
import _localise_miss_spec as MS
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits
from test_gpu_localise_detcov_session import NOISE, covs_of
from test_gpu_localise_session import CLUTTER, DP, GATE, KW, REFINE, compare, scans_and_map

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES, K = 512, 40, 6, 24
LOG_MISS, VIEW_RANGE = -1.5, 6.0
FOV = (-2.351831, 2.351831, 0.05)          # angle_min, angle_max, edge: the reference lidar's arc
SIGHT = (64, 0.4)                          # bins, margin
F = np.float32


def pkg_fov():
    """The arc's bounds as the session makes them: float32 sums, then slam_fov_bound."""
    pkg = load_package()
    return pkg.fov_bound(float(F(FOV[0]) + F(FOV[2]))), pkg.fov_bound(float(F(FOV[1]) - F(FOV[2])))


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    M = np.zeros((5, L), np.float32)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::7] = -1.0                             # slots that hold no landmark, scattered through the map
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def detections(world, f, detcov):
    _, zx, zy = W.observations(world["lm"], 0)
    zx, zy = zx + np.float32(0.01 * f), zy + np.float32(0.01 * f)
    pick = np.random.default_rng(100 + f).permutation(len(zx))[:K]
    zx, zy = zx[pick].copy(), zy[pick].copy()
    return (zx, zy, covs_of(zx, zy)) if detcov else (zx, zy)


def spec_miss(fov, sight, log_miss=LOG_MISS):
    return (log_miss, VIEW_RANGE, pkg_fov() if fov else None, SIGHT if sight else None)


def reference(world, detcov, miss, frames=FRAMES, ess=0.0, refine=None, clutter=CLUTTER, det=None, scans=None, known_map=None):
    kw = {k: v for k, v in KW.items() if k != "meas_var"}
    return MS.frame_loop(world, N, frames, dp=DP, detections=det or (lambda f: detections(world, f, detcov)),
                         known_map=world["M"] if known_map is None else known_map, gate=GATE, log_clutter=clutter,
                         meas_var=None if detcov else KW["meas_var"], miss=miss, ess=ess, refine=refine, scans=scans, **kw)


def open_session(world, ess=0.0, refine=None):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    ses = pkg.PfSession(e, N, 0, resample_ess_frac=ess, **KW)
    if refine:
        ses.refine_set(*refine)
    ses.set_poses(world["x"], world["y"], world["th"])
    return pkg, e, ses


def frame(e, ses, counts=True):
    v = ses.device_view()
    e.sync()
    get = lambda a: torch.as_tensor(a, device=DEV).cpu().numpy()
    fr = dict(pose=ses.poses(), logw=get(v["logw"]), anc=get(v["anc"]) if v["anc"] is not None else None,
              stats=get(ses.known_map_view()["stats"]))
    if counts:
        fr.update({k: get(a) for k, a in ses.known_map_miss_view().items()})
    return fr


def compare_all(g, w, label):
    compare(g, w, label)
    for k in ("missed", "spared", "outside"):
        if w[k] is not None:
            assert np.array_equal(g[k], w[k]), f"{label}: {k}"


def counters(e):
    return dict(miss=e.localise_miss_count(), iso=e.localise_counts()[1], detcov=e.localise_detcov_count(), weight=e.assoc_weight_count(),
                sight=e.sight_counts()[0])


def hand_over(e, world, f, detcov):
    d = detections(world, f, detcov)
    e.detections_upload(d[0], d[1])
    if detcov:
        e.detections_cov_upload(*d[2])


@pytest.mark.parametrize("ess", [0.0, 0.5], ids=["every-frame", "gated"])
@pytest.mark.parametrize("fov,sight", [(False, False), (True, True)], ids=["range", "fov-sight"])
@pytest.mark.parametrize("detcov", [False, True], ids=["iso", "detcov"])
def test_session_equals_the_spec_loop(world, detcov, fov, sight, ess):
    want = reference(world, detcov, spec_miss(fov, sight), ess=ess)
    cnt = {k: sum(int(w[k].sum()) for w in want) for k in ("missed", "spared", "outside")}
    assert cnt["missed"] > 0 and (cnt["outside"] > 0) == fov and sum(int(w["stats"][:, 0].sum()) for w in want) > 0
    pkg, e, ses = open_session(world, ess=ess)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(world["M"], GATE, CLUTTER)
    ses.known_map_miss_set(LOG_MISS, VIEW_RANGE, FOV if fov else None, SIGHT if sight else None)
    c0 = counters(e)
    for f in range(FRAMES):
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare_all(frame(e, ses), want[f], f"frame {f}")
    c1 = counters(e)
    assert {k: c1[k] - c0[k] for k in c0} == dict(miss=FRAMES, iso=0, detcov=0, weight=FRAMES, sight=FRAMES if sight else 0)
    ses.close()
    e.close()


@pytest.mark.parametrize("detcov", [False, True], ids=["iso", "detcov"])
def test_session_with_the_detector_equals_the_spec_loop(world, detcov):
    """Another scan every frame: the detector makes the detections (in its noise form under detcov) and line of sight reads the
    table of that frame's scan; the stage reads the REFINED poses."""
    scans, kws, M = scans_and_map()

    def det(f):
        if detcov:
            zx, zy, q, k, _ = DN.detect_noise(*scans[f], None, NOISE, **kws)
            return zx[:k].copy(), zy[:k].copy(), tuple(v[:k].copy() for v in q)
        zx, zy, k, _ = D.detect(*scans[f], **kws)
        return zx[:k].copy(), zy[:k].copy()

    want = reference(world, detcov, spec_miss(True, True), det=det, scans=scans, known_map=M, refine=REFINE)
    assert sum(int(w["missed"].sum()) for w in want) > 0
    pkg, e, ses = open_session(world, refine=REFINE)
    (ses.known_map_detcov_set if detcov else ses.known_map_set)(M, GATE, CLUTTER)
    if detcov:
        ses.detect_noise_set(NOISE, **kws)
    else:
        ses.detect_set(pkg.DetectParams.default(**kws))
    ses.known_map_miss_set(LOG_MISS, VIEW_RANGE, FOV, SIGHT)
    c0 = counters(e)
    for f in range(FRAMES):
        e.scan_upload(*scans[f])
        ses.step(0, DP, True)
        compare_all(frame(e, ses), want[f], f"frame {f}")
    c1 = counters(e)
    assert c1["miss"] - c0["miss"] == FRAMES and c1["sight"] - c0["sight"] == FRAMES
    ses.close()
    e.close()


@pytest.mark.parametrize("detcov", [False, True], ids=["iso", "detcov"])
def test_switched_on_and_off_between_frames(world, detcov):
    """Frames 0 and 1 without the mode — exactly the launches of a session that never had it — and frame 2 with it, against the
    spec's loop; then by the counters: log_miss = 0 without clutter makes the counts and leaves the weight launch out, replacing
    the map keeps the mode, view_range = 0 switches it off, and switching the map off switches it off for good."""
    def miss(f):
        return spec_miss(True, False) if f == 2 else None

    want = reference(world, detcov, miss, frames=3)
    pkg, e, ses = open_session(world)
    set_map = ses.known_map_detcov_set if detcov else ses.known_map_set
    set_map(world["M"], GATE, CLUTTER)
    plain = "detcov" if detcov else "iso"
    for f in range(3):
        c0 = counters(e)
        if f == 2:
            ses.known_map_miss_set(LOG_MISS, VIEW_RANGE, FOV, None)
        hand_over(e, world, f, detcov)
        ses.step(0, DP, True)
        compare_all(frame(e, ses, counts=miss(f) is not None), want[f], f"frame {f}")
        c1 = counters(e)
        d = {k: c1[k] - c0[k] for k in c0}
        on = miss(f) is not None
        assert d == dict(miss=int(on), iso=int(not on and not detcov), detcov=int(not on and detcov), weight=1, sight=0), (f, d)
    # log_miss = 0 and log_clutter = 0: the counts are made, no weight launch
    set_map(world["M"], GATE, 0.0)                       # replacing the map keeps the mode
    ses.known_map_miss_set(0.0, VIEW_RANGE, FOV, None)
    c0 = counters(e)
    hand_over(e, world, 3, detcov)
    ses.step(0, DP, True)
    c1 = counters(e)
    assert c1["miss"] - c0["miss"] == 1 and c1["weight"] == c0["weight"] and c1[plain] == c0[plain]
    assert int(frame(e, ses)["missed"].sum()) > 0
    ses.known_map_miss_set(0.0, 0.0)                     # view_range == 0: off
    c0 = counters(e)
    hand_over(e, world, 4, detcov)
    ses.step(0, DP, True)
    c1 = counters(e)
    assert c1["miss"] == c0["miss"] and c1[plain] - c0[plain] == 1 and c1["weight"] == c0["weight"]
    ses.known_map_miss_set(LOG_MISS, VIEW_RANGE)
    set_map(None)                                        # the map off: the mode goes off with it ...
    set_map(world["M"], GATE, CLUTTER)                   # ... and a new map does not bring it back
    c0 = counters(e)
    hand_over(e, world, 5, detcov)
    ses.step(0, DP, True)
    c1 = counters(e)
    assert c1["miss"] == c0["miss"] and c1[plain] - c0[plain] == 1 and c1["weight"] - c0["weight"] == 1
    ses.close()
    e.close()


def test_refusals_leave_the_session_as_it_was(world):
    pkg, e, ses = open_session(world)
    with pytest.raises(pkg.SlamError, match="known map") as err:   # no known map
        ses.known_map_miss_set(LOG_MISS, VIEW_RANGE)
    assert err.value.status == -2
    with pytest.raises(pkg.SlamError):
        ses.known_map_miss_view()                                  # never switched on: not ready
    ses.known_map_set(world["M"], GATE, CLUTTER)
    ses.known_map_miss_set(LOG_MISS, VIEW_RANGE, FOV, SIGHT)
    nan, inf = float("nan"), float("inf")
    bad = [dict(log_miss=0.5), dict(log_miss=nan), dict(log_miss=-inf), dict(view_range=-1.0), dict(view_range=inf), dict(view_range=nan),
           dict(fov=(-4.0, 2.0, 0.0)), dict(fov=(-2.0, 4.0, 0.0)), dict(fov=(-1.0, 1.0, 1.0)), dict(fov=(-1.0, 1.0, -0.1)), dict(fov=(nan, 1.0, 0.0)),
           dict(sight=(48, 0.4)), dict(sight=(2048, 0.4)), dict(sight=(64, 0.0)), dict(sight=(64, nan)), dict(sight=(64, inf))]
    c0 = counters(e)
    for kw in bad:
        a = dict(log_miss=LOG_MISS, view_range=VIEW_RANGE, fov=None, sight=None)
        a.update(kw)
        with pytest.raises(pkg.SlamError) as err:
            ses.known_map_miss_set(a["log_miss"], a["view_range"], a["fov"], a["sight"])
        assert err.value.status == -2, kw   # SLAM_ERR_INVALID_ARG
    assert counters(e) == c0
    want = reference(world, False, spec_miss(True, True), frames=1)[0]   # the session is as the accepted call left it
    hand_over(e, world, 0, False)
    ses.step(0, DP, True)
    compare_all(frame(e, ses), want, "after the refusals")
    ses.close()
    e.close()


def test_host_program_charges_the_misses(orc, tmp_path):
    """slam_pf_main --known-map .. --known-miss .. on the head of the recorded dataset runs to completion, in a process of its own
    under its own time limit; the flags without --known-map exit non-zero."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in np.random.default_rng(3).uniform(-8, 8, (20, 2))))
    known = ["--known-map", str(km), "9.21", "0.05", "-2.5", "--detect"]
    for n, extra in enumerate((["--known-miss", "-1.5", "6.0"],
                               ["--known-miss", "-1.5", "6.0", "--known-miss-fov", "0.05", "--known-miss-sight", "64", "0.4"],
                               ["--known-miss", "-1.5", "6.0", "--known-miss-sight", "64", "0.4", "--range-noise", "0.001", "0.00015625", "0.001"])):
        r = subprocess.run(base + [str(tmp_path / f"m{n}.csv"), "256", "3"] + known + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stdout.count("pose =") == len(lines) - 1, (extra, r.stderr)
    r = subprocess.run(base + [str(tmp_path / "m9.csv"), "256", "3", "--known-miss", "-1.5", "6.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    r = subprocess.run(base + [str(tmp_path / "m8.csv"), "256", "3"] + known + ["--known-miss-fov", "0.05"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
    r = subprocess.run(base + [str(tmp_path / "m7.csv"), "256", "3"] + known + ["--known-miss", "0.5", "6.0"], capture_output=True, text=True, timeout=120)
    assert r.returncode != 0
