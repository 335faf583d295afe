"""The fusion of two landmark estimates against the float64 information-form product (P_w^-1 + P_l^-1)^-1 and its forward-error
bounds.  TEST INFRASTRUCTURE shared by test_merge_spec_cpu.py (whose docstring holds the derivation) and the regime tests: one
copy of the formulas.  numpy only."""
import numpy as np

U = 2.0 ** -24


def fusion_check(o, ml, pl, mw, pw, min_use=0.9, label="fusion"):
    """o [5][n] (float64 of the float32 results: mu_x', mu_y', P_xx', P_xy', P_yy') of fusing the absorbed landmarks (means ml
    [2][n], covariances pl [3][n]) into the anchors (mw, pw).  Pairs one of whose rounded inputs lost its definiteness are left
    out; at least min_use of the pairs must remain.  Prints and returns the worst error / bound ratios; asserts them <= 1."""
    mat = lambda p: np.stack([np.stack([p[0], p[1]], -1), np.stack([p[1], p[2]], -1)], -2).astype(np.float64)
    Pl, Pw = mat(pl), mat(pw)
    use = (np.linalg.det(Pl) > 0) & (np.linalg.det(Pw) > 0)           # (a rounded input may have lost its definiteness)
    assert use.mean() > min_use
    Pl, Pw, o = Pl[use], Pw[use], o[:, use]
    mul, muw = ml.astype(np.float64).T[use], mw.astype(np.float64).T[use]
    info = np.linalg.inv(Pw) + np.linalg.inv(Pl)
    P64 = np.linalg.inv(info)
    mu64 = np.einsum("nij,nj->ni", P64, np.einsum("nij,nj->ni", np.linalg.inv(Pw), muw) + np.einsum("nij,nj->ni", np.linalg.inv(Pl), mul))
    S = Pl + Pw
    ev_s = np.linalg.eigvalsh(S)
    lmin, kappa = ev_s[:, 0], ev_s[:, 1] / ev_s[:, 0]
    lmax = lambda m: np.linalg.eigvalsh(m)[:, 1]
    d = np.linalg.norm(mul - muw, axis=1)
    a = np.maximum(1.0, np.linalg.norm(Pl @ np.linalg.inv(S), 2, axis=(1, 2)))
    b_mean = a * U * d + 2 * U * (np.linalg.norm(mul, axis=1) + d) + U * (6 * kappa + 18) * lmax(Pl) * d / lmin
    quad = lambda p: p[:, 0, 0] * p[:, 1, 1] + p[:, 0, 1] ** 2
    b_cov = 4 * U * ((kappa + 2) * lmax(P64) + (lmax(Pl) * quad(Pw) + lmax(Pw) * quad(Pl)) / np.linalg.det(S))
    e_mean = np.linalg.norm(o[:2].T - mu64, axis=1)
    e_cov = np.max(np.abs(np.stack([o[2] - P64[:, 0, 0], o[3] - P64[:, 0, 1], o[4] - P64[:, 1, 1]])), axis=0)
    print(f"{label} vs float64 information form over {use.sum()} pairs: max error / bound  mean {np.max(e_mean / b_mean):.3g}  "
          f"cov {np.max(e_cov / b_cov):.3g}; kappa(S) up to {kappa.max():.3g}")
    assert np.all(e_mean <= b_mean), f"mean: {np.max(e_mean / b_mean):.3g} x its bound"
    assert np.all(e_cov <= b_cov), f"covariance: {np.max(e_cov / b_cov):.3g} x its bound"
    return dict(mean=float(np.max(e_mean / b_mean)), cov=float(np.max(e_cov / b_cov)))
