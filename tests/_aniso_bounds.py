"""The float64 reference of the landmark update with a 2x2 sensor-frame measurement covariance and its forward-error bounds.  TEST
INFRASTRUCTURE shared by test_aniso_spec_cpu.py (whose docstring holds the derivation), test_assoc_aniso_spec_cpu.py,
test_assoc_detcov_spec_cpu.py and the regime tests (test_regimes_spec_cpu.py, test_gpu_regimes.py): one copy of the formulas.
numpy and _f64_pf only."""
import numpy as np

import _f64_pf as F

U, SC = F.U, F.SINCOS_ABS


def q_matrix(qm, ratio, phi):
    """Q with eigenvalues (qm, qm / ratio), the large axis at angle phi, as the float32 triple the interface takes."""
    c, s = np.cos(phi), np.sin(phi)
    lo = qm / ratio
    return tuple(np.float32(v) for v in (qm * c * c + lo * s * s, (qm - lo) * c * s, qm * s * s + lo * c * c))


def world_noise64(cov, th):
    c, s = np.cos(np.asarray(th, np.float64)), np.sin(np.asarray(th, np.float64))
    qxx, qxy, qyy = (float(v) for v in cov)
    return c * c * qxx + 2 * s * c * qxy + s * s * qyy, c * s * (qyy - qxx) + (c * c - s * s) * qxy, s * s * qxx - 2 * s * c * qxy + c * c * qyy


def ekf64(mx, my, pxx, pxy, pyy, zx, zy, px, py, th, cov):
    """The sensor-frame update in float64, per element -> (mu_x', mu_y', P_xx', P_xy', P_yy', ll), diagnostics."""
    f = lambda a: np.asarray(a, np.float64)
    mx, my, pxx, pxy, pyy, zx, zy, px, py, th = map(f, (mx, my, pxx, pxy, pyy, zx, zy, px, py, th))
    qxx, qxy, qyy = (float(v) for v in cov)
    c, s = np.cos(th), np.sin(th)
    h00, h01, h10, h11 = c, -s, s, c
    ex, ey = mx - px, my - py
    vx = zx - (h00 * ex + h01 * ey)
    vy = zy - (h10 * ex + h11 * ey)
    a00, a01 = h00 * pxx + h01 * pxy, h00 * pxy + h01 * pyy      # A = H P
    a10, a11 = h10 * pxx + h11 * pxy, h10 * pxy + h11 * pyy
    s00 = a00 * h00 + a01 * h01 + qxx                            # S = A H^T + Q
    s01 = a00 * h10 + a01 * h11 + qxy
    s11 = a10 * h10 + a11 * h11 + qyy
    dS = s00 * s11 - s01 * s01
    j00, j01, j11 = s11 / dS, -s01 / dS, s00 / dS
    k00, k01 = a00 * j00 + a10 * j01, a00 * j01 + a10 * j11      # K = P H^T S^-1 = A^T S^-1
    k10, k11 = a01 * j00 + a11 * j01, a01 * j01 + a11 * j11
    mux = mx + (k00 * vx + k01 * vy)
    muy = my + (k10 * vx + k11 * vy)
    m00 = 1.0 - (k00 * h00 + k01 * h10)                          # I - K H
    m01 = -(k00 * h01 + k01 * h11)
    m10 = -(k10 * h00 + k11 * h10)
    m11 = 1.0 - (k10 * h01 + k11 * h11)
    o2 = m00 * pxx + m01 * pxy
    o3 = 0.5 * ((m00 * pxy + m01 * pyy) + (m10 * pxx + m11 * pxy))
    o4 = m10 * pxy + m11 * pyy
    maha = vx * (j00 * vx + j01 * vy) + vy * (j01 * vx + j11 * vy)
    ll = -0.5 * maha - 0.5 * np.log(dS) - F.LOG_2PI
    return (mux, muy, o2, o3, o4, ll), dict(s00=s00, s01=s01, s11=s11, vx=vx, vy=vy, maha=maha, dS=dS)


def bounds(prior, pose, zx, zy, cov):
    """The reference's results and the three bounds above for landmarks seen before (arrays that broadcast)."""
    p = [np.asarray(a, np.float64) for a in prior]
    px, py, th = (np.asarray(a, np.float64) for a in pose)
    ref, dg = ekf64(p[0], p[1], p[2], p[3], p[4], zx, zy, px, py, th, cov)
    qxx, qxy, qyy = (float(v) for v in cov)
    _, qm = F._eig2(np.float64(qxx), np.float64(qxy), np.float64(qyy))
    lmin_s, lmax_s = F._eig2(dg["s00"], dg["s01"], dg["s11"])
    _, lmax_p = F._eig2(p[2], p[3], p[4])
    _, lmax_post = F._eig2(ref[2], ref[3], ref[4])
    kap = lmax_s / lmin_s
    e_r = 8.0 * (SC + 2 * U) * qm
    g = 1.0 / (1.0 - 4.0 * e_r / lmin_s)
    assert np.all(g > 0)
    t, mu = np.hypot(px, py), np.hypot(p[0], p[1])
    d = np.hypot(dg["vx"], dg["vy"])
    z = np.hypot(np.asarray(zx, np.float64), np.asarray(zy, np.float64))
    sc = 4.0 * (SC + U) * z
    m = dg["maha"]
    det_p = p[2] * p[4] - p[3] * p[3]
    e_d = 4 * U * (t + mu + d) + sc
    big_d = d + e_d
    # ||P S^-1||_2 in the world frame (S_w = P + R_w has the reference's eigenvalues)
    rw = world_noise64(cov, th)
    w00, w01, w11 = p[2] + rw[0], p[3] + rw[1], p[4] + rw[2]
    dw = w00 * w11 - w01 * w01
    n00, n01 = (p[2] * w11 - p[3] * w01) / dw, (p[3] * w00 - p[2] * w01) / dw
    n10, n11 = (p[3] * w11 - p[4] * w01) / dw, (p[4] * w00 - p[3] * w01) / dw
    _, top = F._eig2(n00 * n00 + n10 * n10, n00 * n01 + n10 * n11, n01 * n01 + n11 * n11)
    a_p = np.maximum(1.0, np.sqrt(top))
    rest = 2 * U * (t + mu + d) + U * (6.0 * kap + 18.0) * qm * big_d / lmin_s + 2 * g * e_r * big_d * (1.0 + qm / lmin_s) / lmin_s
    b_mean = a_p * e_d + rest
    b_cov = (4 * U * ((kap + 2.0) * lmax_post + qm * (p[2] * p[4] + p[3] * p[3]) / dg["dS"])
             + 4 * U * (qxx * qyy + qxy * qxy) * lmax_p / dg["dS"] + g * e_r * (np.abs(det_p) / dg["dS"] + 4.0 * lmax_post / lmin_s))
    b_ll = 8 * U * (kap * (1.0 + m) + np.abs(np.log(dg["dS"])) + 1.0) + 2.0 * np.sqrt(m / lmin_s) * e_d + g * e_r * (m + 2.0) / lmin_s
    return ref, dict(mean=b_mean, mean_normal=e_d + rest, a_p=a_p, cov=b_cov, ll=b_ll, e_r=e_r)


def cov_domain(pxx, pxy, pyy, cov):
    """Where the covariance bound can be checked at all: ekf64 forms P' = (I - K H) P, and the float64 rounding of I - K H (about
    8 * 2^-53 per entry) times P must stay below the bound's leading term 4 u * 3 lambda_max(P') with P' -> Q as P grows:
    lambda_max(P) <= 2^29 lambda_max(Q).  The grid (P / q <= 1e8) lies inside; the ~1e10 m^2 priors do not."""
    _, lmax_p = F._eig2(*(np.asarray(a, np.float64) for a in (pxx, pxy, pyy)))
    _, qm = F._eig2(*(np.float64(v) for v in cov))
    return lmax_p <= 2.0 ** 29 * qm


def check(rows, out, ll, pose, zx, zy, cov, label, groups=None, normal=False, domain=None):
    """One frame with every landmark observed: `out` / `ll` (the spec's, or anything that claims to implement it) against the
    reference and its bounds.  groups: {name: columns}, for the per-regime print.  normal: Q = q I, where P S^-1 is symmetric with
    eigenvalues below 1 — the mean must then meet the bound WITHOUT the factor a_P (a_P = 1): the factor loosens nothing
    there.  domain: bool [n][L], where the covariance is held to its bound (None: everywhere; see cov_domain) — outside it the
    posterior must still be positive definite and no larger than its prior.  -> worst ratios over the frame."""
    n, _, L = rows.shape
    p, g = np.moveaxis(rows, 1, 0), np.moveaxis(out, 1, 0)
    first = p[2] < 0
    seen = ~first
    x, y, th = (np.asarray(a)[:, None] for a in pose)
    pp = np.where(seen, p, np.array([0, 0, 1, 0, 1], np.float32)[:, None, None])
    ref, b = bounds(pp, (x, y, th), zx[None], zy[None], cov)
    r_mean = np.where(seen, np.hypot(g[0] - ref[0], g[1] - ref[1]) / b["mean"], 0.0)
    e_cov = np.maximum(np.maximum(np.abs(g[2] - ref[2]), np.abs(g[3] - ref[3])), np.abs(g[4] - ref[4]))
    r_cov = np.where(seen if domain is None else seen & domain, e_cov / b["cov"], 0.0)
    g64 = [a.astype(np.float64) for a in g]
    pd = (g64[2] > 0) & (g64[4] > 0) & (g64[2] * g64[4] - g64[3] * g64[3] > 0)
    # never larger than the prior: P - P' is positive semidefinite up to the bound on P' (its entries: the eigenvalue by twice that)
    d_lo, _ = F._eig2(pp[2] - g64[2], pp[3] - g64[3], pp[4] - g64[4])
    shrinks = np.where(seen, d_lo >= -2.0 * b["cov"], True)
    # first sightings: the observed point, P = R_w
    fx, fy = F.first_sighting(zx[None], zy[None], x, y, th)
    b_first = 4 * U * (np.hypot(x, y) + np.hypot(fx, fy)) + 4 * (SC + U) * np.hypot(zx, zy)[None]
    r_first = np.where(first, np.hypot(g[0] - fx, g[1] - fy) / b_first, 0.0)
    rw = world_noise64(cov, th)
    e_first = np.maximum(np.maximum(np.abs(g[2] - rw[0]), np.abs(g[3] - rw[1])), np.abs(g[4] - rw[2]))
    r_first = np.maximum(r_first, np.where(first, e_first / b["e_r"], 0.0))
    ll64 = np.where(seen, ref[5], 0.0)
    b_sum = np.where(seen, b["ll"], 0.0).sum(axis=1) + (-(-L // 128) + 7) * U * np.abs(ll64).sum(axis=1) + 1e-30
    r_ll = np.abs(np.asarray(ll, np.float64) - ll64.sum(axis=1)) / b_sum
    for name, cols in (groups or {}).items():
        print(f"{label} {name}: max error / bound  mean {r_mean[:, cols].max():.3g}  cov {r_cov[:, cols].max():.3g}  "
              f"first {r_first[:, cols].max():.3g}")
    worst = dict(mean=float(r_mean.max()), cov=float(r_cov.max()), first=float(r_first.max()), loglik=float(r_ll.max()))
    a_max = float(np.where(seen, b["a_p"], 1.0).max())
    if normal:
        worst["mean without a_P"] = float(np.where(seen, np.hypot(g[0] - ref[0], g[1] - ref[1]) / b["mean_normal"], 0.0).max())
        assert a_max <= 1.0 + 1e-9, f"{label}: ||P S^-1|| = {a_max} with an isotropic Q"
    print(f"{label}: largest a_P = max(1, ||P S^-1||_2) {a_max:.4g}" + (f"; mean error / bound without a_P {worst['mean without a_P']:.3g}" if normal else ""))
    print(f"{label}: max error / bound  mean {worst['mean']:.3g}  cov {worst['cov']:.3g}  first {worst['first']:.3g}  "
          f"loglik {worst['loglik']:.3g}; not positive definite {int((~pd & seen).sum())}; larger than the prior {int((~shrinks).sum())}")
    for k, v in worst.items():
        assert v <= 1.0, f"{label}: {k} error {v:.3g} x its bound"
    assert pd[seen].all(), f"{label}: posteriors not positive definite"
    assert shrinks.all(), f"{label}: posteriors larger than their priors"
    return worst


def check_pairs(rows, out, ll, pose, cols, dx, dy, covs, label=""):
    """One frame in which landmark cols[k] of every particle took detection k = (dx[k], dy[k]) under its own Q_k = covs[k] and the
    other landmarks took none: the bounds above pair by pair with each pair's own quantities (test_assoc_detcov_spec_cpu.py's
    docstring), the particle's log-likelihood against the sum of its pairs' bounds plus the (ceil(L / 128) + 7) u sum |ll| of the
    summation tree.  rows / out [n][5][L].  Prints and returns the worst ratios (and the largest a_P); asserts them <= 1 and every
    posterior positive definite."""
    n, _, L = rows.shape
    x, y, th = pose
    worst = dict(mean=0.0, cov=0.0, first=0.0)
    ll64, b_sum, a_max = np.zeros(n), np.zeros(n), 1.0
    for k in range(len(cols)):
        l = cols[k]
        p, g = rows[:, :, l].T.astype(np.float64), out[:, :, l].T.astype(np.float64)
        first = p[2] < 0
        seen = ~first
        pp = np.where(seen, p, np.array([0, 0, 1, 0, 1], np.float64)[:, None])
        ref, b = bounds(pp, (x, y, th), dx[k], dy[k], covs[k])
        worst["mean"] = max(worst["mean"], float(np.where(seen, np.hypot(g[0] - ref[0], g[1] - ref[1]) / b["mean"], 0.0).max()))
        e_cov = np.maximum(np.maximum(np.abs(g[2] - ref[2]), np.abs(g[3] - ref[3])), np.abs(g[4] - ref[4]))
        worst["cov"] = max(worst["cov"], float(np.where(seen, e_cov / b["cov"], 0.0).max()))
        assert np.all(((g[2] > 0) & (g[4] > 0) & (g[2] * g[4] - g[3] * g[3] > 0))[seen]), f"k={k}: posteriors not positive definite"
        fx, fy = F.first_sighting(dx[k], dy[k], x, y, th)
        b_first = 4 * U * (np.hypot(x, y) + np.hypot(fx, fy)) + 4 * (SC + U) * np.hypot(dx[k], dy[k])
        rw = world_noise64(covs[k], th)
        e_first = np.maximum(np.maximum(np.abs(g[2] - rw[0]), np.abs(g[3] - rw[1])), np.abs(g[4] - rw[2]))
        r_first = np.maximum(np.hypot(g[0] - fx, g[1] - fy) / b_first, e_first / b["e_r"])
        worst["first"] = max(worst["first"], float(np.where(first, r_first, 0.0).max()))
        t = np.where(seen, ref[5], 0.0)
        ll64 += t
        b_sum += np.where(seen, b["ll"], 0.0) + (-(-L // 128) + 7) * U * np.abs(t)
        a_max = max(a_max, float(np.where(seen, b["a_p"], 1.0).max()))
    worst["loglik"] = float((np.abs(np.asarray(ll, np.float64) - ll64) / (b_sum + 1e-30)).max())
    print(f"{label}: max error / bound  mean {worst['mean']:.3g}  cov {worst['cov']:.3g}  first {worst['first']:.3g}  "
          f"loglik {worst['loglik']:.3g}; largest a_P {a_max:.4g}")
    for name, v in worst.items():
        assert v <= 1.0, f"{name} error {v:.3g} x its bound"
    return worst
