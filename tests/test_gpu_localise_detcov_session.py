"""A session without maps of its own that localises in ONE known landmark map under the covariance each detection carries
(slam_pf_known_map_detcov_set) against the frame loop of tests/_localise_detcov_spec.py, frame by frame and bit for bit: poses,
log-weights, ancestors and the stage's stats — with uploaded detections and covariances, a frame without observations and a
switch-off mid-run; with the detector in its noise form, which only this switch accepts; alternating the two known-map switches;
the frame whose detections carry no covariance; the launch counters; and slam_pf_main --known-map --detect --range-noise."""
import subprocess

import numpy as np
import pytest

import _detect_noise_spec as DN
import _localise_detcov_spec as SD
import _localise_spec as S
import oracle
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN
from test_gpu_localise_session import CLUTTER, DP, FRAMES, GATE, KW, N, compare, detections, frame, open_session, scans_and_map, world   # noqa: F401 - world is a fixture

pytestmark = pytest.mark.gpu
RANGE_VAR, BEARING_VAR, LATERAL_VAR = 0.01, 0.002, 0.005
NOISE = (1e-3, 1.5625e-4, 1e-3)
KW_SPEC = {k: v for k, v in KW.items() if k != "meas_var"}


def covs_of(zx, zy):
    """Q_k = a u u^T + b v v^T of each detection: a = RANGE_VAR along its line of sight, b = BEARING_VAR r^2 + LATERAL_VAR across."""
    zx, zy = zx.astype(np.float64), zy.astype(np.float64)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = RANGE_VAR, BEARING_VAR * r2 + LATERAL_VAR
    return tuple(v.astype(np.float32) for v in (a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux))


def feed(world, f):
    zx, zy = detections(world, f)
    return zx, zy, covs_of(zx, zy)


def reference(world, known_map, frames=FRAMES, clutter=CLUTTER, det=None, scans=None):
    return SD.frame_loop(world, N, frames, dp=DP, detections=det or (lambda f: feed(world, f)), known_map=known_map, gate=GATE,
                         log_clutter=clutter, scans=scans, **KW_SPEC)


def hand_over(e, world, f):
    zx, zy, covs = feed(world, f)
    e.detections_upload(zx, zy)
    e.detections_cov_upload(*covs)


def counters(e):
    return e.localise_detcov_count(), e.localise_counts(), e.assoc_weight_count()


@pytest.mark.parametrize("clutter", [CLUTTER, 0.0], ids=["clutter", "no-clutter"])
def test_session_equals_the_spec_loop(world, clutter):
    """Frames 0, 1 and 3 localise, frame 2 has use_observations = 0, in front of frame 4 the mode is switched off."""
    observing = lambda f: f != 2
    want = reference(world, lambda f: world["M"] if f < 4 else None, clutter=clutter, det=lambda f: feed(world, f) if observing(f) else None)
    st = np.stack([want[f]["stats"] for f in (0, 1, 3)])
    assert 0 < st[..., 0].sum() < st[..., [0, 2]].sum() and np.all(st[..., 1] == 0)   # matches and unmatched detections
    pkg, e, ses = open_session(world)
    c0 = counters(e)
    ses.known_map_detcov_set(world["M"], GATE, clutter)
    v = ses.known_map_view()
    assert v["prepared"] is None and v["nlandmarks"] == world["M"].shape[1]
    for f in range(FRAMES):
        if f == 4:
            ses.known_map_detcov_set(None)
            assert ses.known_map_view()["nlandmarks"] == 0
        hand_over(e, world, f)
        ses.step(0, DP, observing(f))
        compare(frame(e, ses, stats=observing(f) and f < 4), want[f], f"frame {f}")
    c1 = counters(e)
    assert c1[0] - c0[0] == 3 and c1[1] == c0[1] and c1[2] - c0[2] == (3 if clutter else 0)   # no prepare launch, no isotropic stage
    ses.close()
    e.close()


def test_session_with_the_detectors_noise_model(world):
    """The detector in its noise form is accepted only under the new switch; detections and covariances come from each frame's scan."""
    scans, kws, M = scans_and_map()

    def det(f):
        zx, zy, q, k, _ = DN.detect_noise(*scans[f], None, NOISE, **kws)
        return zx[:k].copy(), zy[:k].copy(), tuple(v[:k].copy() for v in q)

    want = reference(world, M, det=det, scans=scans)
    assert min(len(det(f)[0]) for f in range(FRAMES)) >= 3 and sum(int(w["stats"][:, 0].sum()) for w in want) > 0
    pkg, e, ses = open_session(world)
    ses.known_map_set(M, GATE, CLUTTER)
    with pytest.raises(pkg.SlamError, match="meas_var"):
        ses.detect_noise_set(NOISE, **kws)
    ses.known_map_detcov_set(M, GATE, CLUTTER)
    ses.detect_noise_set(NOISE, **kws)
    d0, n0, c0 = e.detect_count(), e.detect_noise_count(), counters(e)
    for f in range(FRAMES):
        e.scan_upload(*scans[f])
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f}")
    c1 = counters(e)
    assert e.detect_count() - d0 == FRAMES and e.detect_noise_count() - n0 == FRAMES
    assert c1[0] - c0[0] == FRAMES and c1[1] == c0[1] and c1[2] - c0[2] == FRAMES
    ses.close()
    e.close()


def test_alternating_the_two_switches(world):
    """Either switch replaces the other from the next frame on: every frame is the frame of the form that is on, from the same
    state — poses, weights and ancestors carry over, the stats are those of the stage that ran."""
    M = world["M"]
    form = lambda f: "detcov" if f % 2 == 0 else "iso"
    pkg, e, ses = open_session(world)
    c0 = counters(e)
    got = []
    for f in range(FRAMES):
        (ses.known_map_detcov_set if form(f) == "detcov" else ses.known_map_set)(M, GATE, CLUTTER)
        assert (ses.known_map_view()["prepared"] is None) == (form(f) == "detcov")
        hand_over(e, world, f)
        ses.step(0, DP, True)
        got.append(frame(e, ses))
    c1 = counters(e)
    assert c1[0] - c0[0] == FRAMES // 2 and tuple(np.subtract(c1[1], c0[1])) == (FRAMES // 2, FRAMES // 2)
    ses.close()
    e.close()
    # the reference: one state carried through the two specifications' stages in turn (every frame resamples: no carry)
    x, y, th = (np.ascontiguousarray(world[k][:N]) for k in ("x", "y", "th"))
    anc = None
    for f in range(FRAMES):
        x, y, th = oracle.motion_sample(x, y, th, anc, N, 0, DP, KW["sigma"], KW["seed"], f)
        sc, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        zx, zy, covs = feed(world, f)
        if form(f) == "detcov":
            _, stats, ll = SD.localise(M, x, y, th, zx, zy, covs, GATE, CLUTTER)
        else:
            _, stats, ll = S.localise(M, x, y, th, zx, zy, KW["meas_var"], GATE, CLUTTER)
        logw, m = oracle.logweight_carry(sc, ll, KW["score_gain"], None)
        wq, _ = oracle.quantise_weights(logw, m)
        anc = oracle.resample(wq, KW["seed"], f)
        compare(got[f], dict(pose=np.stack([x[anc], y[anc], th[anc]]), logw=logw, anc=anc, stats=stats), f"frame {f} ({form(f)})")


def test_a_frame_without_covariances_launches_nothing(world):
    """Detections without covariances, and the detector without a model: SLAM_ERR_NOT_READY before the first launch, no counter
    moves, and the good frames behind it are the spec's from the start."""
    want = reference(world, world["M"], frames=2)
    pkg, e, ses = open_session(world)
    ses.known_map_detcov_set(world["M"], GATE, CLUTTER)
    c0, d0 = counters(e), e.detect_count()
    e.detections_upload(*detections(world, 0))
    for _ in range(2):
        with pytest.raises(pkg.SlamError) as err:
            ses.step(0, DP, True)
        assert err.value.status == -4 and "carry none" in str(err.value), str(err.value)
    hand_over(e, world, 0)
    ses.detect_set()                                                     # a detector without a model installs detections without
    with pytest.raises(pkg.SlamError) as err:
        ses.step(0, DP, True)
    assert err.value.status == -4
    ses.detect_set(None)
    e.sync()
    assert counters(e) == c0 and e.detect_count() == d0
    for f in range(2):
        hand_over(e, world, f)
        ses.step(0, DP, True)
        compare(frame(e, ses), want[f], f"frame {f} behind the refused frames")
    ses.close()
    e.close()


def test_refusals(world):
    pkg = load_package()
    M = world["M"]

    def changed(p, l, v):
        B = M.copy()
        B[p, l] = v
        return B

    _, e, ses = open_session(world)
    for text, call in (("gate", lambda s: s.known_map_detcov_set(M, 0.0, 0.0)), ("gate", lambda s: s.known_map_detcov_set(M, float("nan"), 0.0)),
                       ("log_clutter", lambda s: s.known_map_detcov_set(M, GATE, 0.5)),
                       ("not finite", lambda s: s.known_map_detcov_set(changed(0, 1, np.nan), GATE, 0.0)),
                       ("semi-definite", lambda s: s.known_map_detcov_set(changed(4, 3, -0.5), GATE, 0.0)),      # P_yy < 0
                       ("semi-definite", lambda s: s.known_map_detcov_set(changed(3, 4, 10.0), GATE, 0.0))):     # det P < 0
        with pytest.raises(pkg.SlamError, match=text) as err:
            call(ses)
        assert err.value.status == -2, text
    flat = changed(4, 3, 0.0)
    flat[3, 3] = 0.0
    ses.known_map_detcov_set(flat, GATE, 0.0)                 # P_yy == 0 = P_xy: semi-definite is enough, every Q_k is definite
    ses.close()
    e.close()
    _, e, ses = open_session(world, n_landmarks=8, layout="rows")
    with pytest.raises(pkg.SlamError, match="n_landmarks == 0"):
        ses.known_map_detcov_set(M, GATE, CLUTTER)
    ses.close()
    e.close()


def test_host_program_with_range_noise(orc, tmp_path):
    """slam_pf_main --known-map --detect --range-noise on the head of the recorded dataset runs to completion; --range-noise
    without --detect, and the combinations --known-map forbids, exit non-zero."""
    exe = PKG_DIR / "lib" / "slam_pf_main"
    csv = GOLDEN / "frames_head.csv"
    lines = csv.read_text().splitlines()
    base = [str(exe), str(csv), str(len(lines)), str(len(lines[1].split(",")))]
    km = tmp_path / "known.csv"
    km.write_text("".join(f"{x:f},{y:f}\n" for x, y in np.random.default_rng(3).uniform(-8, 8, (20, 2))))
    known = ["--known-map", str(km), "9.21", "0.05", "-2.5"]
    noise = ["--detect", "--range-noise", "0.0004", "0.0002", "0.0004"]
    r = subprocess.run(base + [str(tmp_path / "m0.csv"), "256", "3"] + known + noise, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.count("pose =") == len(lines) - 1, r.stderr
    r = subprocess.run(base + [str(tmp_path / "m1.csv"), "256", "3"] + known + noise[1:], capture_output=True, text=True, timeout=120)
    assert r.returncode == 2                                             # only with --detect
    for extra in (["--landmarks", "16"], ["--gpus", "2", "--transport", "local", "--same-device"], ["--meas-cov", "0.02", "0", "0.03"]):
        r = subprocess.run(base + [str(tmp_path / "m2.csv"), "256", "3"] + known + noise + extra, capture_output=True, text=True, timeout=120)
        assert r.returncode != 0, extra
