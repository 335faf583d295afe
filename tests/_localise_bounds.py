"""The textbook Gaussian log-likelihood of a particle's matched pairs in a known map, in float64, and the relative bound the
localise specification is held to.  TEST INFRASTRUCTURE of test_localise_spec_cpu.py, kept beside the other stages' bound helpers.
The regime tests do not use it: at |pose| = 1e3 the relative bound below is outside its domain, and they
hold each matched pair to the update's own log-likelihood bound instead (_regimes.localise_check).  numpy only."""
import numpy as np

REL = 1e-5    # |ll - ll_64| <= REL |ll_64| (test_localise_spec_cpu.py: unit-scale covariances, poses of a few metres)


def textbook(M, q, x, y, th, zx, zy, pairs):
    """sum over (l, k) of -1/2 d^T S^-1 d - 1/2 log det S - log 2 pi in float64; M [5][L] the known map, S = P_l + q I."""
    c, s = np.cos(float(th)), np.sin(float(th))
    ll = 0.0
    for l, k in pairs:
        w = np.array([float(x) + c * float(zx[k]) + s * float(zy[k]), float(y) + c * float(zy[k]) - s * float(zx[k])])
        Sm = np.array([[M[2, l], M[3, l]], [M[3, l], M[4, l]]], np.float64) + float(np.float32(q)) * np.eye(2)
        d = w - M[:2, l].astype(np.float64)
        ll += -0.5 * d @ np.linalg.solve(Sm, d) - 0.5 * np.log(np.linalg.det(Sm)) - np.log(2 * np.pi)
    return ll


def within(ll, want):
    return abs(float(ll) - want) <= REL * abs(want)
