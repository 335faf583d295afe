"""Global localisation with the specification's frame loop (tests/_localise_spec.py, score = False: a drive without a grid): a
cloud drawn uniformly over a known map of poles, with uniform headings, finds the robot from nothing but the poles it detects;
the same loop without the map can only diffuse.  The bound on the error: profiles/localise.md."""
import numpy as np
import pytest

import _localise_spec as S

F = np.float32
N, FRAMES, POLES = 3000, 24, 20
HALF, VIEW = 10.0, 7.0                    # the poles lie in [-HALF, HALF]^2; the sensor sees those within VIEW metres
MAP_VAR, GATE, CLUTTER = 0.25, 9.21, -6.0
KW = dict(sigma=(0.08, 0.08, 0.03), meas_var=0.01, score_gain=0.0)
SEED = 1
BOUND = 0.0174                            # metres: twice the worst of seeds 1 .. 5 (0.0087 m, seed 2; profiles/localise.md)


def scene(seed):
    """-> (M [5][POLES], truth [FRAMES + 1][3] along an arc, dp(f), detections(f), the cloud x, y, th)."""
    rng = np.random.default_rng(seed)
    M = np.zeros((5, POLES), np.float32)
    M[0], M[1] = rng.uniform(-HALF, HALF, POLES), rng.uniform(-HALF, HALF, POLES)   # scattered at random: no rotational symmetry
    M[2], M[4] = MAP_VAR, MAP_VAR
    truth = np.zeros((FRAMES + 1, 3))
    truth[0] = (-3.0, -2.0, 0.4)
    for f in range(FRAMES):               # an arc: 0.25 m and 0.06 rad a frame
        th = truth[f, 2]
        truth[f + 1] = truth[f] + (0.25 * np.cos(th), 0.25 * np.sin(th), 0.06)
    dps = np.diff(truth, axis=0).astype(F)

    def detections(f):                    # what pose f + 1 sees: z = H (m - t), 2 cm of noise
        px, py, th = truth[f + 1]
        dx, dy = M[0] - px, M[1] - py
        near = np.hypot(dx, dy) < VIEW
        c, s = np.cos(th), np.sin(th)
        nz = np.random.default_rng(1000 * seed + f).normal(0, 0.02, (2, int(near.sum())))
        return (c * dx[near] - s * dy[near] + nz[0]).astype(F), (s * dx[near] + c * dy[near] + nz[1]).astype(F)

    x = rng.uniform(M[0].min(), M[0].max(), N).astype(F)
    y = rng.uniform(M[1].min(), M[1].max(), N).astype(F)
    th = rng.uniform(-np.pi, np.pi, N).astype(F)
    return M, truth, (lambda f: dps[f]), detections, dict(x=x, y=y, th=th)


def final_error(seed, on):
    """Position error of the population's mean at the last frame (every frame resamples: the resampled population's plain mean
    is its weighted mean)."""
    M, truth, dp, detections, cloud = scene(seed)
    out = S.frame_loop(cloud, N, FRAMES, seed=seed, dp=dp, detections=detections, known_map=M if on else None, gate=GATE,
                       log_clutter=CLUTTER, score=False, **KW)
    est = out[-1]["pose"][:2].astype(np.float64).mean(axis=1)
    return float(np.hypot(*(est - truth[FRAMES, :2])))


@pytest.fixture(scope="module")
def errors(orc):
    return final_error(SEED, True), final_error(SEED, False)


def test_the_cloud_finds_the_robot(errors):
    on, off = errors
    print(f"position error at the last frame: {on:.4f} m with the known map, {off:.4f} m without")
    assert on < off
    assert on < BOUND
