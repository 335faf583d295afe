"""slam_pf_spread restated exactly (include/slam_hip.h): the mean of tests/_estimate_spec.py, then the second
moments of the population about it as exact sums of Python integers.  numpy, Python integers and the oracle's deterministic
functions; nothing of the package under test.  TEST INFRASTRUCTURE."""
import math
import operator

import numpy as np

import oracle
from _estimate_spec import mean_spec, trunc_div, trunc_fixed

D_SHIFT = 20                      # DX, DY, SS = trunc(. * 2^20)
DOMAIN = np.float32(2048.0)       # |dx|, |dy| < 2048 m
PAIRS = ((0, 0), (0, 1), (1, 1), (0, 2), (1, 2), (2, 2))   # cov[k]: xx, xy, yy, xs, ys, ss


class OutOfDomain(ValueError):
    """A particle lies 2048 m or more from the mean in x or y: the call refuses (SLAM_ERR_INVALID_ARG)."""


def deltas(x, y, th, idx, pose, cast=trunc_fixed):
    """-> (DX, DY, SS) as lists of Python integers, the particles behind the gather idx, about the float32 mean `pose`."""
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    if idx is not None:
        idx = np.asarray(idx, np.int64)
        x, y, th = x[idx], y[idx], th[idx]
    mx, my, mt = (np.float32(v) for v in pose)
    dx, dy = (x - mx).astype(np.float32), (y - my).astype(np.float32)          # one binary32 subtraction each
    s, _ = oracle.det_sincos((th - mt).astype(np.float32))                       # one more, then the specified polynomial
    if not (np.all(np.abs(dx) < DOMAIN) and np.all(np.abs(dy) < DOMAIN)):        # (a NaN is outside as well)
        raise OutOfDomain
    return cast(dx, D_SHIFT), cast(dy, D_SHIFT), cast(s, D_SHIFT)


def moment_sums(x, y, th, idx, pose, w16=None, cast=trunc_fixed):
    """-> ([six sums of w A B], sum w) of these particles about `pose`; w = 1 without w16.  Sums of shards add."""
    d = deltas(x, y, th, idx, pose, cast)
    w = [1] * len(d[0]) if w16 is None else [int(v) for v in w16]
    assert len(w) == len(d[0])
    wd = [list(map(operator.mul, w, a)) for a in d]
    return [sum(map(operator.mul, wd[i], d[j])) for i, j in PAIRS], sum(w)


def cov_from_sums(sums, d):
    """cov[k] = float32(float64(trunc(sum_k / D)) / 2^40)"""
    return np.array([np.float32(float(trunc_div(t, d)) / 2.0 ** 40) for t in sums], np.float32)


def heading_r(ss, sc, d):
    """length of the mean heading vector from the mean's own sums: hypot(trunc(sum S / D), trunc(sum C / D)) / 2^30"""
    return np.float32(math.hypot(float(trunc_div(ss, d)), float(trunc_div(sc, d))) / 2.0 ** 30)


def spread_spec(x, y, th, idx, ref_theta, n_total, w16=None, cast=trunc_fixed):
    """-> (pose float32 [3], cov float32 [6], heading_r float32, (the six sums, D)); raises OutOfDomain.
    w16 None (or without any weight): the plain form, D = n_total; else the weighted form of a frame the gate kept."""
    if w16 is not None and sum(int(v) for v in w16) <= 0:
        w16 = None
    pose, ms = mean_spec(x, y, th, idx, ref_theta, n_total, w16)
    sums, d = moment_sums(x, y, th, idx, pose, w16, cast)
    if w16 is None:
        d = int(n_total)
    return pose, cov_from_sums(sums, d), heading_r(ms[2], ms[3], d), (sums, d)


def f64_cov(x, y, th, pose, w=None):
    """float64 covariance over (x, y, sin(theta - pose[2])) about `pose`, population form -> [6] in the order of PAIRS"""
    x, y, th = (np.asarray(a, np.float32).astype(np.float64) for a in (x, y, th))
    w = np.ones(len(x)) if w is None else np.asarray(w, np.float64)
    d = [x - float(pose[0]), y - float(pose[1]), np.sin(th - float(pose[2]))]
    return np.array([(w * d[i] * d[j]).sum() / w.sum() for i, j in PAIRS])


# ------------------------------------------------------------------ the pose populations the spread's tests add
def spread_population(name, n, seed=0):
    """-> (x, y, th) float32 [n]"""
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    if name == "two_clusters":       # 8 m apart with opposite headings: heading_r near 0, the covariance is that of the pair
        side = np.arange(n) % 2
        x = (np.where(side == 0, -4.0, 4.0) + rng.normal(0, 0.01, n)).astype(np.float32)
        y = rng.normal(1.0, 0.01, n).astype(np.float32)
        th = (np.where(side == 0, 0.5, 0.5 + np.pi) + rng.normal(0, 0.01, n)).astype(np.float32)
    elif name == "far_cloud":        # 1 cm across, 1000 m out: a cast before the centring would leave nothing of it
        x = (1000.0 + rng.normal(0, 0.01, n)).astype(np.float32)
        y = (-1000.0 + rng.normal(0, 0.01, n)).astype(np.float32)
        th = rng.normal(2.0, 0.01, n).astype(np.float32)
    elif name == "off_grid":         # most deltas negative and all off the 2^-20 grid (sizes below 2^-3 carry bits under 2^-20, and so
        # do sines below 2^-3): a few large positive ones pull the mean up, so that truncation and floor differ in most terms
        x = (rng.uniform(0.0, 0.06, n) + np.where(np.arange(n) % 16 == 0, 0.5, 0.0)).astype(np.float32)
        y = (-rng.uniform(0.0, 0.03, n) + np.where(np.arange(n) % 16 == 0, 0.25, 0.0)).astype(np.float32)
        th = (rng.uniform(-0.05, 0.0, n) + np.where(np.arange(n) % 16 == 0, 0.1, 0.0)).astype(np.float32)
    elif name == "identical":
        x, y, th = (np.full(n, v, np.float32) for v in (0.1, -1e-7, 3.0))
    else:
        raise KeyError(name)
    return x, y, th


def boundary_population(n, far, seed=0):
    """a tight cloud with ONE particle `far` metres from the rest in x (2047.9: just inside the domain for n > 20 481; 2048.1: outside)"""
    rng = np.random.default_rng([seed, n, 99])
    x = rng.normal(1.0, 0.05, n).astype(np.float32)
    y = rng.normal(-2.0, 0.05, n).astype(np.float32)
    th = rng.normal(0.3, 0.02, n).astype(np.float32)
    x[n // 3] = np.float32(1.0 + far)
    return x, y, th
