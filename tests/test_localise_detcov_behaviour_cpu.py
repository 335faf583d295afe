"""Global localisation under the lidar's own noise with the specification's frame loop (tests/_localise_detcov_spec.py,
score = False): the scene of test_localise_behaviour_cpu.py — 20 poles, 3 000 particles spread over the map, 24 frames — with the
detections' noise DRAWN FROM THE DETECTOR'S RANGE MODEL (range_var along the beam, bearing_var r^2 + lateral_var across it: a pole
7 m away is 9 cm uncertain across the beam, one 1 m away 1.6 cm) and every detection fed with its own Q_k.  The bound on the error,
and the same scene under the isotropic stage with one best-guess meas_var: profiles/localise_detcov.md."""
import numpy as np

import _localise_detcov_spec as SD
import _localise_spec as S
from test_localise_behaviour_cpu import CLUTTER, FRAMES, GATE, HALF, MAP_VAR, N, POLES, VIEW

F = np.float32
RANGE_VAR, BEARING_VAR, LATERAL_VAR = 1e-4, 1.5625e-4, 1e-4   # 1 cm in range; 12.5 mrad in bearing and 1 cm across the beam
KW = dict(sigma=(0.08, 0.08, 0.03), score_gain=0.0)
ISO_VAR = 0.01                            # the isotropic stage's single guess: the across-beam variance at 4 m, mid-view
SEED = 1
# metres: twice the worst of seeds 1 .. 5 (profiles/localise_detcov.md).  The worst is seed 5, whose cloud settles on a wrong pose
# 7.5 m away under this form AND under the isotropic one (seeds 1 .. 4: 0.7 to 2.6 cm): by the rule the bound is this wide, and what
# the test can still hold the form to beside it is that the map helps at all
BOUND = 15.0384


def model_cov(zx, zy):
    """Q_k of the detections (float64 here, rounded once: the inputs of the filter, not the thing under test)."""
    zx, zy = np.asarray(zx, np.float64), np.asarray(zy, np.float64)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = RANGE_VAR, BEARING_VAR * r2 + LATERAL_VAR
    return tuple(v.astype(F) for v in (a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux))


def scene(seed):
    """test_localise_behaviour_cpu.scene with the detections' noise drawn from the model.
    -> (M [5][POLES], truth [FRAMES + 1][3], dp(f), detections(f) -> (zx, zy, Q), the cloud x, y, th)."""
    rng = np.random.default_rng(seed)
    M = np.zeros((5, POLES), np.float32)
    M[0], M[1] = rng.uniform(-HALF, HALF, POLES), rng.uniform(-HALF, HALF, POLES)
    M[2], M[4] = MAP_VAR, MAP_VAR
    truth = np.zeros((FRAMES + 1, 3))
    truth[0] = (-3.0, -2.0, 0.4)
    for f in range(FRAMES):               # an arc: 0.25 m and 0.06 rad a frame
        th = truth[f, 2]
        truth[f + 1] = truth[f] + (0.25 * np.cos(th), 0.25 * np.sin(th), 0.06)
    dps = np.diff(truth, axis=0).astype(F)

    def detections(f):                    # what pose f + 1 sees: z = H (m - t), noise along and across each line of sight
        px, py, th = truth[f + 1]
        dx, dy = M[0] - px, M[1] - py
        near = np.hypot(dx, dy) < VIEW
        c, s = np.cos(th), np.sin(th)
        z = np.stack([c * dx[near] - s * dy[near], s * dx[near] + c * dy[near]], axis=1)
        r = np.hypot(z[:, 0], z[:, 1])
        u = z / r[:, None]
        nz = np.random.default_rng(1000 * seed + f).standard_normal((2, len(z)))
        along, across = np.sqrt(RANGE_VAR) * nz[0], np.sqrt(BEARING_VAR * r * r + LATERAL_VAR) * nz[1]
        z = z + along[:, None] * u + across[:, None] * np.stack([-u[:, 1], u[:, 0]], axis=1)
        zx, zy = z[:, 0].astype(F), z[:, 1].astype(F)
        return zx, zy, model_cov(zx, zy)

    x = rng.uniform(M[0].min(), M[0].max(), N).astype(F)
    y = rng.uniform(M[1].min(), M[1].max(), N).astype(F)
    th = rng.uniform(-np.pi, np.pi, N).astype(F)
    return M, truth, (lambda f: dps[f]), detections, dict(x=x, y=y, th=th)


def final_error(seed, form):
    """Position error of the population's mean at the last frame; form: "per detection", "isotropic" (the same detections
    without their covariances, meas_var = ISO_VAR) or "off" (no map: the cloud can only diffuse)."""
    M, truth, dp, detections, cloud = scene(seed)
    common = dict(seed=seed, dp=dp, known_map=M if form != "off" else None, gate=GATE, log_clutter=CLUTTER, score=False, **KW)
    if form == "per detection":
        out = SD.frame_loop(cloud, N, FRAMES, detections=detections, **common)
    else:
        out = S.frame_loop(cloud, N, FRAMES, detections=lambda f: detections(f)[:2], meas_var=ISO_VAR, **common)
    est = out[-1]["pose"][:2].astype(np.float64).mean(axis=1)
    return float(np.hypot(*(est - truth[FRAMES, :2])))


def test_the_cloud_finds_the_robot_under_the_lidars_noise(orc):
    _, truth, _, detections, _ = scene(SEED)
    zx, zy, q = detections(FRAMES - 1)
    r = np.hypot(zx, zy)
    far, near = np.argmax(r), np.argmin(r)
    # (the inputs are what the scene was chosen for: the far pole is visibly noisier than the near one)
    assert (q[0][far] + q[2][far]) > 4 * (q[0][near] + q[2][near])
    err, off = final_error(SEED, "per detection"), final_error(SEED, "off")
    print(f"position error at the last frame: {err:.4f} m under per-detection covariances, {off:.4f} m without the map")
    assert err < off
    assert err < BOUND
