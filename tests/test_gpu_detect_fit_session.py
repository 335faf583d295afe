"""A rows session with the fitted detector on (slam_pf_assoc_set + slam_pf_detect_fit_set, with and without slam_pf_prune_set)
against the frame loop of tests/_detect_spec.py fed tests/_detect_fit_spec.py's detections, over ray-cast frames with a different
scan each: poses, maps, log-weights, ancestors, association tables and evidence bit for bit; switching the fit off mid-run returns
to the centroid session's bits; the fit is refused where slam_pf_detect_set is; and slam_pf_main --pole-radius."""
import subprocess

import numpy as np
import pytest
import torch

import _detect_fit_spec as DF
import _detect_spec as D
import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 256, 16, 8
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 3, 4.0)
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]
RHO, HALF = 0.1, 5.0
FIT = (RHO, 0.0)
POLES = np.random.default_rng(12).uniform(-4.0, 4.0, (12, 2))


def scan(f):
    """Frame f: the pole room as the moving sensor sees it, 360 beams with 1 cm of range noise — another scan every frame."""
    pose = (f + 1) * np.array(DP)
    bx, by, _, _ = D.raycast(pose, POLES, RHO, HALF, 360, noise=np.random.default_rng(900 + f))
    return bx, by


SCANS = [scan(f) for f in range(FRAMES)]


def fitted(f):
    zx, zy, k, _ = DF.detect_fit(*SCANS[f], FIT)
    return zx[:k].copy(), zy[:k].copy()


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, _, _, _ = W.make_world(L=L)
    x, y, th, _ = W.init_state(N, 0, np.zeros((0, 2), np.float32))
    mp = np.zeros((N, 5, L), np.float32)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), x=x, y=y, th=th, mp=mp)


@pytest.fixture(scope="module")
def want(world):
    """The spec loops, computed once: (fit | centroid) x (assoc | pruning)."""
    loop = lambda det, prune: D.frame_loop(world, SCANS, N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=prune, detections=det, **KW)
    return {("fit", None): loop(fitted, None), ("fit", PRUNE): loop(fitted, PRUNE), ("centroid", PRUNE): loop(None, PRUNE)}


def open_session(world, layout="rows", assoc=True, prune=None):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    ses = pkg.PfSession(e, N, L, map_layout=layout, **KW)
    if assoc:
        ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"][:N], world["y"][:N], world["th"][:N])
    ses.set_map(world["mp"][:N])
    if prune:
        ses.prune_set(*prune)
    return e, ses


def frame(e, ses, prune):
    v = ses.device_view()
    av = ses.assoc_view()
    e.sync()
    fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
              anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy(),
              assoc=torch.as_tensor(av["assoc"], device=DEV).cpu().numpy(), stats=torch.as_tensor(av["stats"], device=DEV).cpu().numpy())
    if prune:
        fr["ev"] = ses.evidence()
    return fr


def compare(g, w, label, prune):
    assert np.array_equal(g["assoc"][:, :L], w["assoc"][:, :L]), f"{label}: association table"
    assert np.array_equal(g["stats"], w["stats"]), f"{label}: association stats"
    assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label}: log-weights"
    assert np.array_equal(g["anc"], w["anc"]), f"{label}: ancestors"
    assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label}: poses"
    assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label}: map rows"
    if prune:
        assert np.array_equal(g["ev"], w["ev"]), f"{label}: evidence"


@pytest.mark.parametrize("prune", [None, PRUNE], ids=["assoc", "pruning"])
def test_session_equals_the_spec_loop(world, want, prune):
    w = want[("fit", prune)]
    c = want[("centroid", PRUNE)]
    assert min(len(f["det"][0]) for f in w) >= 3 and len(set(bits(f["det"][0]).tobytes() for f in w)) == FRAMES
    assert all(not np.array_equal(bits(a["det"][0]), bits(b["det"][0])) for a, b in zip(w, c))       # the fit moves the detections
    assert sum(int(f["stats"][:, 1].sum()) for f in w) > 0 and int(w[-1]["stats"][:, 0].sum()) > 0   # landmarks made, then matched
    e, ses = open_session(world, prune=prune)
    ses.detect_fit_set(FIT)
    c0, f0, a0, v0 = e.detect_count(), e.detect_fit_count(), e.assoc_counts(), e.evidence_counts()
    for f in range(FRAMES):
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, prune), w[f], f"frame {f}", prune)
        zx, zy = e.detections()
        assert np.array_equal(bits(zx), bits(w[f]["det"][0])) and np.array_equal(bits(zy), bits(w[f]["det"][1]))
    # one detector launch per frame, each of them a fit, in front of the same associate and update (and evidence) launches
    assert e.detect_count() - c0 == FRAMES and e.detect_fit_count() - f0 == FRAMES
    assert tuple(np.subtract(e.assoc_counts(), a0)) == (FRAMES, FRAMES)
    assert tuple(np.subtract(e.evidence_counts(), v0)) == ((FRAMES, 0) if prune else (0, 0))
    ses.step(0, DP, False)                       # a frame without observations launches no detector
    assert e.detect_count() - c0 == FRAMES
    ses.close()
    e.close()


@pytest.mark.parametrize("how", ["detect_set", "fit=None"])
def test_switching_the_fit_off_returns_to_the_centroid_session(world, want, how):
    """Frames 0-3 of a centroid session; the same with the fit switched on and off again before frame 0 — by slam_pf_detect_set, by
    slam_pf_detect_fit_set(params, NULL) — and, at the end, slam_pf_assoc_set(0) clears the fit with the detector."""
    w = want[("centroid", PRUNE)]
    e, ses = open_session(world, prune=PRUNE)
    ses.detect_fit_set(FIT)
    if how == "detect_set":
        ses.detect_set()
    else:
        ses.detect_fit_set(None)
    f0 = e.detect_fit_count()
    for f in range(4):
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, PRUNE), w[f], f"frame {f}", PRUNE)
    assert e.detect_fit_count() == f0
    ses.detect_fit_set(FIT)
    ses.assoc_set(0.0)                           # association off: the detector and its fit go with it, and stay off
    ses.assoc_set(GATE, NEW_GATE, True)
    c0 = e.detect_count()
    e.detections_upload(*w[0]["det"])
    ses.step(0, DP, True)
    assert e.detect_count() == c0 and e.detect_fit_count() == f0
    ses.detect_set()                             # ... and a detector switched on afterwards is the centroid detector
    e.scan_upload(*SCANS[0])
    ses.step(0, DP, True)
    assert e.detect_count() == c0 + 1 and e.detect_fit_count() == f0
    ses.close()
    e.close()


def test_mid_run_switch(world, want):
    """Frames 0-3 with the fit, then off: frames 4-7 are those of a session fed the fitted detections for four frames and the
    centroid detector's afterwards."""
    mixed = lambda f: fitted(f) if f < 4 else (lambda r: (r[0][:r[2]].copy(), r[1][:r[2]].copy()))(D.detect(*SCANS[f]))
    w = D.frame_loop(world, SCANS, N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, detections=mixed, **KW)
    e, ses = open_session(world, prune=PRUNE)
    ses.detect_fit_set(FIT)
    for f in range(FRAMES):
        if f == 4:
            ses.detect_set()
            f4 = e.detect_fit_count()
        e.scan_upload(*SCANS[f])
        ses.step(0, DP, True)
        compare(frame(e, ses, PRUNE), w[f], f"frame {f}", PRUNE)
    assert e.detect_fit_count() == f4
    ses.close()
    e.close()


@pytest.mark.parametrize("case", ["association off", "split", "bad parameters", "bad fit"])
def test_refusals(world, case):
    """... and the session then steps exactly as one that was never asked."""
    pkg = load_package()
    ids = np.arange(5, dtype=np.int32)
    z = np.linspace(-2, 2, 5).astype(np.float32)
    out = []
    for ask in (False, True):
        e, ses = open_session(world, layout="split" if case == "split" else "rows", assoc=case.startswith("bad"))
        if ask:
            if case == "split":
                with pytest.raises(pkg.SlamError):
                    ses.assoc_set(GATE, NEW_GATE, True)
            with pytest.raises(pkg.SlamError) as err:
                if case == "bad parameters":
                    ses.detect_fit_set(FIT, min_points=0)
                elif case == "bad fit":
                    ses.detect_fit_set((0.0, 0.0))
                else:
                    ses.detect_fit_set(FIT)
            assert err.value.status == -2
            word = {"bad parameters": "min_points", "bad fit": "radius"}.get(case, "data association")
            assert word in str(err.value), str(err.value)
        frames = []
        for f in range(2):
            e.scan_upload(*SCANS[f])
            e.obs_upload(ids, z, z[::-1].copy(), L)
            e.detections_upload(z, z)
            ses.step(0, DP, True)
            frames.append((ses.poses(), ses.maps()))
        assert e.detect_count() == 0 and e.detect_fit_count() == 0
        out.append(frames)
        ses.close()
        e.close()
    for f in range(2):
        for g, w in zip(out[1][f], out[0][f]):
            assert np.array_equal(bits(g), bits(w)), f"{case}: frame {f}"


def test_host_program_pole_radius(orc, tmp_path):
    """slam_pf_main --detect ... --pole-radius 0.1 on a ring of poles seen by the program's own sensor: the map file's landmarks lie
    nearer their poles' centres than a run without it leaves them; --pole-radius without --detect is refused with the usage text."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    ring = np.deg2rad(30.0 * np.arange(12) + 3.0)
    poles = np.stack([(3.0 + 0.1 * np.arange(12)) * np.cos(ring), (3.0 + 0.1 * np.arange(12)) * np.sin(ring)], 1)
    ang = -2.351831 + 0.004363 * np.arange(1079)
    rng = D.raycast((0.0, 0.0, 0.0), poles, RHO, 6.0, angles=ang)
    ranges = np.hypot(rng[0].astype(np.float64), rng[1].astype(np.float64))
    room = tmp_path / "room.csv"
    room.write_text("".join(",".join(f"{v:.6f}" for v in ranges) + "\n" for _ in range(4)))
    base = [str(exe), str(room), "4", "1079", str(tmp_path / "map_room.csv"), "256", "3", "--landmarks", "32", "--assoc", "9.21", "50"]
    det = ["--detect", "0.3", "1.0", "0.5", "20", "3", "40", "0"]
    rms = {}
    for name, extra in (("centroid", []), ("fit", ["--pole-radius", "0.1"]), ("fit_tol", ["--pole-radius", "0.1", "0.02"])):
        lm = tmp_path / f"{name}.csv"
        r = subprocess.run(base + det + extra + ["--landmarks-out", str(lm)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        found = np.array([[float(v) for v in ln.split(",")] for ln in lm.read_text().splitlines()])
        d = np.hypot(found[:, None, 0] - poles[None, :, 0], found[:, None, 1] - poles[None, :, 1]).min(axis=1)
        rms[name] = float(np.sqrt(np.mean(d ** 2)))
        assert len(found) == DF.detect_fit(rng[0], rng[1], FIT if extra else None, wrap=0)[2] >= 3
    print(rms)
    # the filter's poses lie within centimetres of the origin after three frames of 1 cm motion noise: 0.05 m covers them, and the
    # centroid's own bias (0.08 m and more of the radius at this resolution) does not fit under it
    assert rms["fit"] < 0.05 < rms["centroid"] and rms["fit_tol"] < 0.05
    r = subprocess.run(base + ["--pole-radius", "0.1"], capture_output=True, text=True)
    assert r.returncode == 2 and "--pole-radius" in r.stderr
    r = subprocess.run(base + det + ["--pole-radius", "-1"], capture_output=True, text=True)
    assert r.returncode != 0 and "radius" in r.stderr
