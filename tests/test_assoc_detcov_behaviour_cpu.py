"""Does the filter that associates under a covariance per detection (tests/_assoc_detcov_spec.py: frame_loop) grow the right map
when the poles stand ALL ROUND the sensor, at 1 to 15 m, and the noise is truly a lidar's — drawn from the range / bearing model,
range_var << bearing_var r^2 —, 20 % of the detections are missed, every frame brings one false detection and pruning is on?
One sensor-frame Q per session is right for one bearing and one range only; here every detection carries
Q_k = a u u^T + b v v^T, a = range_var, b = bearing_var r^2 + lateral_var, along and across its own line of sight.
profiles/assoc_detcov.md records what this filter, the best single-Q one found and the isotropic one do on the same drive over
five seeds; only what the inputs were chosen for is asserted: the heaviest particle ends with exactly one landmark per true pole
and none spurious (a landmark: a slot whose evidence has reached CONFIRMED, the notion of test_evidence_behaviour_cpu.py).  No GPU."""
import numpy as np

import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _assoc_spec as A
import _evidence_spec as E
from test_assoc_behaviour_cpu import map_error

N, L_TRUE, SLOTS, FRAMES = 256, 12, 24, 40
KW = dict(sigma=(0.01, 0.01, 0.002), score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
DP = (0.05, 0.005, 0.002)
RANGE_VAR, BEARING_VAR, LATERAL_VAR = 1e-4, 1.5625e-4, 1e-4   # 1 cm in range; 12.5 mrad in bearing and 1 cm across the beam
MISSED = 0.2
PRUNE = (1, 1, 8, 20.0)                                       # hit, miss, cmax, view_range: every pole is always in view
CONFIRMED = 4                                                 # evidence from which a slot counts as a landmark: half of cmax


def model_cov(zx, zy):
    """Q_k of the detections (float64 here, rounded once: the inputs of the filter, not the thing under test)."""
    zx, zy = np.asarray(zx, np.float64), np.asarray(zy, np.float64)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = RANGE_VAR, BEARING_VAR * r2 + LATERAL_VAR
    return tuple(v.astype(np.float32) for v in (a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux))


def drive(seed=42):
    """12 poles all round the sensor, 1 to 15 m from the start and at least 1 m apart; the true trajectory (the noise-free motion
    model from the origin); per frame the poles seen (20 % missed), each at its true range and bearing plus noise DRAWN FROM THE
    MODEL (range: RANGE_VAR; across the beam: BEARING_VAR r^2 + LATERAL_VAR), and one false detection anywhere in the annulus, in
    shuffled order.  -> (poles [12][2], per frame (zx, zy, (qxx, qxy, qyy)))."""
    rng = np.random.default_rng(seed)
    lm = []
    while len(lm) < L_TRUE:
        r, b = rng.uniform(1.0, 15.0), rng.uniform(-np.pi, np.pi)
        p = np.array([r * np.cos(b), r * np.sin(b)])
        if all(np.hypot(*(p - o)) >= 1.0 for o in lm):
            lm.append(p)
    lm = np.array(lm)
    pose, frames = np.zeros(3), []
    for f in range(FRAMES):
        pose = pose + np.array(DP)
        c, s = np.cos(pose[2]), np.sin(pose[2])
        d = lm - pose[:2]
        z = np.stack([c * d[:, 0] + s * d[:, 1], c * d[:, 1] - s * d[:, 0]], axis=1)       # H (m - t), H^T = [[c, s], [-s, c]]
        r = np.hypot(z[:, 0], z[:, 1])
        u = z / r[:, None]
        along = np.sqrt(RANGE_VAR) * rng.standard_normal(L_TRUE)
        across = np.sqrt(BEARING_VAR * r * r + LATERAL_VAR) * rng.standard_normal(L_TRUE)
        z = z + along[:, None] * u + across[:, None] * np.stack([-u[:, 1], u[:, 0]], axis=1)
        ids = np.flatnonzero(rng.random(L_TRUE) >= MISSED)
        fr, fb = rng.uniform(1.0, 15.0), rng.uniform(-np.pi, np.pi)
        z = np.concatenate([z[ids], [[fr * np.cos(fb), fr * np.sin(fb)]]])[rng.permutation(len(ids) + 1)]
        zx, zy = z[:, 0].astype(np.float32), z[:, 1].astype(np.float32)
        frames.append((zx, zy, model_cov(zx, zy)))
    return lm, frames


def confirmed_map(out, lm):
    """The heaviest particle of the last frame (it survives the resample): its landmarks are the slots in use whose evidence has
    reached CONFIRMED — a false detection of the last frames holds a slot until its misses have used up its one hit.
    -> (landmarks, distinct true poles they are nearest to, RMS distance to those)."""
    last = out[-1]
    k = int(np.flatnonzero(last["anc"] == np.argmax(last["logw"]))[0])
    row = last["map"][k].copy()
    row[2, last["ev"][k] < CONFIRMED] = -1.0
    return map_error(row, lm)


def fresh_world():
    world = dict(x=np.zeros(N, np.float32), y=np.zeros(N, np.float32), th=np.zeros(N, np.float32), mp=np.zeros((N, 5, SLOTS), np.float32))
    world["mp"][:, 2] = -1.0
    return world


def run(kind, seed, q=None):
    """-> (landmarks, distinct true poles among them, RMS distance to them) of the heaviest particle of the last frame."""
    lm, frames = drive(42 + seed)
    common = dict(dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, score=False, prune=PRUNE, seed=5 + seed, **KW)
    if kind == "per detection":
        out = AD.frame_loop(fresh_world(), N, FRAMES, detections=lambda f: frames[f], **common)
    elif kind == "one Q":
        out = AA.frame_loop(fresh_world(), N, FRAMES, detections=lambda f: frames[f][:2], meas_cov=q, **common)
    else:
        out = E.frame_loop(fresh_world(), N, FRAMES, detections=lambda f: frames[f][:2], meas_var=q, **common)
    return confirmed_map(out, lm)


def test_one_landmark_per_pole_and_none_spurious(orc):
    for seed in range(5):
        seen, distinct, rms = run("per detection", seed)
        print(f"seed {seed}, per detection: {seen} landmarks, {distinct} distinct poles, rms {rms:.4f} m")
        assert seen == distinct == L_TRUE, (seed, seen, distinct)
