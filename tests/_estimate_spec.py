"""What a host takes out of a particle-filter session, restated exactly: the posterior mean (slam_pf_mean: pose_sums_kernel plus
the host arithmetic of pf_mean) and the heaviest particle (slam_pf_best: best_particle_kernel / argmax_kernel).  DESIGN.md
section 7.  numpy, Python integers and the oracle's deterministic functions; nothing of the package under test.
TEST INFRASTRUCTURE."""
import math

import numpy as np

import oracle

XY_SHIFT, SC_SHIFT = 32, 30


def trunc_fixed(a, shift):
    """trunc(a * 2^shift) per element as Python integers.  A float32 times a power of two is exact in float64, and the cast of
    C truncates towards zero."""
    v = np.trunc(np.asarray(a, np.float32).astype(np.float64) * 2.0 ** shift)
    return [int(t) for t in v.tolist()]


def floor_fixed(a, shift):
    """The same with floor: what the kernel must NOT compute (the negative-coordinates case tells the two apart)."""
    v = np.floor(np.asarray(a, np.float32).astype(np.float64) * 2.0 ** shift)
    return [int(t) for t in v.tolist()]


def trunc_div(a: int, b: int) -> int:
    """a / b as C divides integers: towards zero (b > 0)."""
    return a // b if a >= 0 else -((-a) // b)


def weights16(logw):
    """The 16-bit weights of a frame and its 32-bit ones: w16 = quantise(det_exp(logw - max)) >> 16, the integers the resample
    gate's S and Q are made of (oracle.quantise_weights, oracle.ess_terms).  The maximum ignores NaN, as fmaxf does."""
    logw = np.ascontiguousarray(logw, np.float32)
    m = np.float32(np.fmax.reduce(logw, initial=np.float32(-np.inf)))
    wq, _ = oracle.quantise_weights(logw, m)
    return [int(w) >> 16 for w in wq.tolist()], wq


def gate_resamples(wq, n_total, frac_q16):
    """The resample gate's verdict on a frame's quantised weights (True: the frame resamples)."""
    if not frac_q16:
        return True
    s16, q16 = oracle.ess_terms(wq)
    return oracle.ess_resample(s16, q16, n_total, frac_q16)


def mean_spec(x, y, th, idx, ref_theta, n_total, w16=None):
    """-> (float32 [x, y, theta], the raw sums).  idx: the pending gather (slot i holds particle idx[i]) or None.
    w16 None: the plain mean, sums = (sum X, sum Y, sum S, sum C).
    w16 (one integer per slot): the weighted mean of a frame the gate kept, sums = (sum w X, sum w Y, sum w S, sum w C, D)."""
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    if idx is not None:
        idx = np.asarray(idx, np.int64)
        x, y, th = x[idx], y[idx], th[idx]
    ref = np.float32(ref_theta)
    s, c = oracle.det_sincos((th - ref).astype(np.float32))   # one binary32 subtraction, then the specified polynomial
    fixed = [trunc_fixed(x, XY_SHIFT), trunc_fixed(y, XY_SHIFT), trunc_fixed(s, SC_SHIFT), trunc_fixed(c, SC_SHIFT)]
    if w16 is None:
        sx, sy, ss, sc = (sum(v) for v in fixed)
        nt = float(n_total)
        pose = [np.float32(float(sx) / 2.0 ** 32 / nt), np.float32(float(sy) / 2.0 ** 32 / nt),
                np.float32(float(ref) + math.atan2(float(ss), float(sc)))]
        return np.array(pose, np.float32), (sx, sy, ss, sc)
    w = [int(v) for v in w16]
    assert len(w) == len(x)
    d = sum(w)
    sums = [sum(wi * vi for wi, vi in zip(w, v)) for v in fixed]
    qx, qy, qs, qc = (trunc_div(t, d) for t in sums)
    pose = [np.float32(float(qx) / 2.0 ** 32), np.float32(float(qy) / 2.0 ** 32),
            np.float32(float(ref) + math.atan2(float(qs), float(qc)))]
    return np.array(pose, np.float32), (*sums, d)


def best_spec(logw, x, y, th, first_id=0):
    """-> (float32 [x, y, theta], log-weight, global index): the largest log-weight, the lowest index on ties; NaN never wins;
    when every value is -inf or NaN: index 0 with value -inf."""
    logw = np.ascontiguousarray(logw, np.float32)
    best_v, best_i = -math.inf, 0
    for i, v in enumerate(logw.tolist()):
        if v > best_v:          # false for NaN, and for the later one of two equal values
            best_v, best_i = v, i
    pose = np.array([x[best_i], y[best_i], th[best_i]], np.float32)
    return pose, np.float32(best_v), int(first_id) + best_i


# ------------------------------------------------------------------ the pose populations the tests share
# ref_theta per population: up to +-pi off it; 3.0 / 9.0 / -2.5 / -3.0: theta - ref passes the range reduction of det_sincos (|a| >= pi/4)
REFS = {"plain": [0.0, 0.07, 3.0, -math.pi, 9.0], "straddle_pi": [math.pi, 3.0, 0.0, -2.5], "negative": [0.0, 1.0, -3.0],
        "large": [0.0, -0.8]}


def edge_population(name, n, seed=0):
    """Pose populations on the edges the estimates can get wrong -> (x, y, th) float32 [n]."""
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    x = rng.normal(0.5, 0.3, n).astype(np.float32)
    y = rng.normal(-0.25, 0.3, n).astype(np.float32)
    th = rng.normal(0.0, 0.05, n).astype(np.float32)
    if name == "plain":
        pass
    elif name == "straddle_pi":      # headings on both sides of +-pi: their arithmetic mean is near 0, the circular one near pi
        th = (np.where(np.arange(n) % 2 == 0, np.pi - 0.2, -np.pi + 0.2) + rng.normal(0, 0.05, n)).astype(np.float32)
    elif name == "negative":         # negative and OFF the fixed-point grids, so that truncation and floor differ: a binary32 below
        # 2^-8 in size has bits under 2^-32 (x, y), a sine below 2^-6 has bits under 2^-30 (headings just below ref = 0)
        x = (-np.abs(rng.normal(0.0, 1.0, n)) * 2.0 ** -10 - 1e-5).astype(np.float32)
        y = (-np.abs(rng.normal(0.0, 1.0, n)) * 2.0 ** -12 - 1e-7).astype(np.float32)
        th = (-np.abs(rng.normal(0.0, 0.003, n)) - 1e-4).astype(np.float32)
    elif name == "large":            # n * max|x| just inside the 64-bit limit of the plain sum, all of one sign
        top = np.float32(2.0 ** 31 / n * 0.999)
        x = (top * rng.uniform(0.98, 1.0, n)).astype(np.float32)
        y = (-top * rng.uniform(0.98, 1.0, n)).astype(np.float32)
    else:
        raise KeyError(name)
    return x, y, th


def f64_means(x, y, th, ref_theta, w=None):
    """float64 mean of x and y and the float64 circular mean -> (mx, my, theta, r): r = length of the mean heading vector."""
    x, y, th = (np.asarray(a, np.float32).astype(np.float64) for a in (x, y, th))
    w = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    d = th - float(np.float32(ref_theta))
    ms, mc = (w * np.sin(d)).sum() / w.sum(), (w * np.cos(d)).sum() / w.sum()
    return (w * x).sum() / w.sum(), (w * y).sum() / w.sum(), float(np.float32(ref_theta)) + math.atan2(ms, mc), math.hypot(ms, mc)


# ------------------------------------------------------------------ gated scenarios (resample_ess_frac in (0, 1))
SIGMA, SEED, DP = (0.02, 0.02, 0.004), 77, (0.01, -0.005, 0.002)
# n, ess, steps before the break, what breaks the run of frames ("set_poses" / "reset"), steps after it
GATED_SCENARIOS = {4097: dict(ess=0.5, gain=0.1, first=8, then="set_poses", rest=2),
                   65537: dict(ess=0.5, gain=0.1, first=8, then="reset", rest=2)}
RESET_POSE = (0.1, -0.2, 0.03)


def gated_oracle_run(world, x, y, th, n, ess, first, then, rest, gain=1.0):
    """The gated frame loop of a session without landmarks, written with the oracle's functions ->
    one record per event: ("step", resampled, plain mean, weighted mean) or (then, None, plain mean, None).
    world: (meta, edt, bx, by) of tests/_shard_worker.make_world."""
    meta, edt, bx, by = world
    fq = oracle.ess_frac_q16(ess)
    out = []

    def steps(x, y, th, count):
        anc, carry, prev_resampled = None, None, True
        for f in range(count):
            x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, list(DP), SIGMA, SEED, frame[0])
            frame[0] += 1
            score, _ = oracle.score_poses_det(meta, edt, bx, by, x, y, th)
            logw, m = oracle.logweight_carry(score, None, gain, None if prev_resampled else carry)
            w16, wq = weights16(logw)
            prev_resampled = gate_resamples(wq, n, fq)
            carry = oracle.weight_carry(logw, m)
            anc = oracle.resample(wq, SEED, frame[0] - 1) if prev_resampled else np.arange(n, dtype=np.int32)
            ref = float(np.float32(th.mean()))
            plain, _ = mean_spec(x, y, th, anc, ref, n)
            weighted, _ = mean_spec(x, y, th, anc, ref, n, w16)
            out.append(("step", prev_resampled, plain, weighted))
        return x[anc], y[anc], th[anc]

    frame = [0]
    x, y, th = steps(x, y, th, first)
    if then == "reset":
        x, y, th = (np.full(n, v, np.float32) for v in RESET_POSE)
        frame[0] = 0
    else:
        x, y, th = x[::-1].copy(), y[::-1].copy(), th[::-1].copy()   # what the test hands to set_poses: the population, reversed
    out.append((then, None, mean_spec(x, y, th, None, 0.0, n)[0], None))
    steps(x, y, th, rest)
    return out
