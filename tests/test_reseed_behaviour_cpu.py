"""What reseeding is for, on the specification's frame loop (tests/_reseed_spec.py frame_loop, score = False: a drive without a
grid; no GPU): the sensor of tests/_pipeline_scenes.py drives through a room of poles, one ray-cast scan and one run of the
fitted detector per frame, and at JUMP_FRAME the true pose jumps by more than 10 m and 90 degrees while the odometry says nothing.
Without a reseed the cloud never leaves the old track; with fraction 1/16 behind every frame it comes back; and a cloud parked at
the origin (the same drive without the jump: a start nobody told the filter) finds the robot from fraction 1 behind its first
frame and 1/16 from there on.  The tolerance is measured, not chosen: twice the steady-state error of the same loop,
map, seed and drive WITHOUT the jump (the recovered cloud is a fresh one that has had fewer frames to settle).  Per-seed figures:
profiles/reseed.md."""
import functools

import numpy as np
import pytest

import _detect_fit_spec as DF
import _detect_spec as D
import _pipeline_scenes as P
import _reseed_spec as R

F = np.float32
N, FRAMES, JUMP_FRAME = 2048, 32, 3
HALF = 12.0                                    # the room [-HALF, HALF]^2
JUMP = (9.0, 6.0, 2.0)                         # metres, metres, radians: 10.8 m and 115 degrees
STEADY = range(FRAMES - 5, FRAMES)             # the frames of the reference run whose largest error is the steady-state error
MAP_VAR, GATE, CLUTTER = 0.05, 9.21, -6.0
KW = dict(sigma=(0.08, 0.08, 0.03), meas_var=0.01, score_gain=0.0)
SEEDS = (1, 2, 3, 4, 5, 6, 7, 8)
# the scenes' seven poles and five more towards the corners the jump lands in: scattered, no rotational symmetry
POLES = np.concatenate([P.POLES, np.array([(6.5, 5.0), (8.0, 1.5), (5.0, 8.5), (-6.0, 4.5), (-4.5, -6.5)], np.float64)])


def truth(jump):
    """[FRAMES + 1][3]: 0.2 m and 0.04 rad a frame from (-3, -3, 0.3); with jump, pose JUMP_FRAME + 1 onwards is displaced by JUMP."""
    t = np.zeros((FRAMES + 1, 3))
    t[0] = (-3.0, -3.0, 0.3)
    for f in range(FRAMES):
        t[f + 1] = t[f] + (0.2 * np.cos(t[f, 2]), 0.2 * np.sin(t[f, 2]), 0.04)
    if jump:
        t[JUMP_FRAME + 1:] += JUMP
    return t


@functools.lru_cache(maxsize=None)
def scene(jump):
    """-> (M [5][L], truth, dp [FRAMES][3] — the odometry never reports the jump —, detections [FRAMES] of (zx, zy))."""
    M = np.zeros((5, len(POLES)), F)
    M[0], M[1], M[2], M[4] = POLES[:, 0], POLES[:, 1], MAP_VAR, MAP_VAR
    t = truth(jump)
    dp = np.diff(truth(False), axis=0).astype(F)
    det = []
    for f in range(FRAMES):
        # the project's pose convention: a sensor-frame point is z = H(theta) (w - t) with H = [[c, -s], [s, c]]
        bx, by, _, _ = D.raycast((t[f + 1, 0], t[f + 1, 1], t[f + 1, 2]), POLES, P.RHO, HALF, noise=np.random.default_rng(100 + f), angles=P.ANGLES)
        zx, zy, k, _ = DF.detect_fit(bx, by, P.FIT, **dict(P.PARAMS))   # the fitted detector: a pole's centre, from wherever it is seen
        det.append((zx[:k].copy(), zy[:k].copy()))
    return M, t, dp, det


def errors(seed, jump, fraction, parked=False):
    """Position error of the population's mean after every frame, as a host reads it: with the frame's resample applied, BEFORE
    the reseed behind the frame (whose proposals, scattered over the map, are weighed by the next frame).  fraction: None, a
    number (behind every frame), or a function of the frame."""
    M, t, dp, det = scene(jump)
    rng = np.random.default_rng(seed)
    start = np.zeros(3) if parked else t[0]
    cloud = dict(x=np.full(N, start[0], F), y=np.full(N, start[1], F), th=np.full(N, start[2], F))
    if not parked:
        cloud["x"] += (0.1 * rng.standard_normal(N)).astype(F)
        cloud["y"] += (0.1 * rng.standard_normal(N)).astype(F)
    out = R.frame_loop(cloud, N, FRAMES, seed=seed, dp=lambda f: dp[f], detections=lambda f: det[f], known_map=M, gate=GATE,
                       log_clutter=CLUTTER, score=False, reseed_after=fraction if callable(fraction) or fraction is None else (lambda f: fraction), **KW)
    est = np.stack([w["pose"][:2].astype(np.float64).mean(axis=1) for w in out])
    return np.hypot(*(est - t[1:, :2]).T)


@functools.lru_cache(maxsize=None)
def case(seed):
    """-> dict of the four runs' error curves and the tolerance of this seed: twice the largest error of the reference run (no jump,
    no reseed) over the frames of STEADY."""
    ref = errors(seed, False, None)
    return dict(ref=ref, tol=2.0 * float(ref[list(STEADY)].max()), lost=errors(seed, True, None), back=errors(seed, True, 1.0 / 16),
                parked=errors(seed, False, lambda f: 1.0 if f == 0 else 1.0 / 16, parked=True))


def recovered_at(err, tol, first):
    """The first frame from `first` on behind which the error stays within tol to the end (None: never)."""
    bad = np.flatnonzero(err[first:] > tol)
    at = first if len(bad) == 0 else first + int(bad[-1]) + 1
    return at if at < len(err) else None


def test_the_scene_holds_what_the_test_is_about(orc):
    M, t, dp, det = scene(True)
    assert np.hypot(*JUMP[:2]) >= 10.0 and JUMP[2] >= np.pi / 2 and np.all(np.abs(t[:, :2]) < HALF - 1.0)
    assert min(len(d[0]) for d in det) >= 3 and min(len(d[0]) for d in scene(False)[3]) >= 3   # every frame sees poles


@pytest.mark.parametrize("seed", SEEDS)
def test_without_a_reseed_the_cloud_stays_lost(orc, seed):
    c = case(seed)
    half = 0.5 * float(np.hypot(*JUMP[:2]))
    print(f"seed {seed}: errors behind the jump, no reseed: min {c['lost'][JUMP_FRAME:].min():.2f} m, last {c['lost'][-1]:.2f} m (half the jump: {half:.2f} m)")
    assert np.all(c["lost"][JUMP_FRAME:] > half)


@pytest.mark.parametrize("seed", SEEDS)
def test_reseeding_brings_the_cloud_back(orc, seed):
    c = case(seed)
    at = recovered_at(c["back"], c["tol"], JUMP_FRAME)
    print(f"seed {seed}: tolerance {c['tol']:.4f} m (steady state {c['tol'] / 2:.4f} m); back within it behind frame {at} "
          f"({None if at is None else at - JUMP_FRAME} frames after the jump); last error {c['back'][-1]:.4f} m")
    assert at is not None, "the mean does not return and stay within the tolerance to the end"


@pytest.mark.parametrize("seed", SEEDS)
def test_a_parked_cloud_finds_the_robot_from_fraction_one(orc, seed):
    c = case(seed)
    at = recovered_at(c["parked"], c["tol"], 0)
    print(f"seed {seed}: parked at the origin, fraction 1: within {c['tol']:.4f} m behind frame {at}; last error {c['parked'][-1]:.4f} m")
    assert at is not None, "the mean does not reach the tolerance and stay within it to the end"
