"""The specification of the landmark update with a 2x2 sensor-frame measurement covariance (tests/_aniso_spec.py) against an
independent float64 reference — the textbook EKF in the SENSOR frame,
    H = [[c, -s], [s, c]],  nu = z - H (mu - t),  S = H P H^T + Q,  K = P H^T S^-1,  mu' = mu + K nu,  P' = (I - K H) P,
    ll = -1/2 nu^T S^-1 nu - 1/2 log det S - log 2 pi,
every 2 x 2 product written out on whole arrays — and the properties a user relies on.  No GPU.

FORWARD-ERROR BOUNDS (the style of _f64_pf.update_errors; u = 2^-24; qm = lambda_max(Q); S = P + R_w in the world frame, where it
has the eigenvalues of the sensor-frame S; kappa(S), lambda_min(S); d the innovation; w = t + H^T z; m = d^T S^-1 d).

  The rounding of R_w.  Every entry of R_w = H^T Q H is a quadratic form c^2 qxx + 2 s c qxy + s^2 qyy (or its kin) whose
  gradient in (s, c) is at most 2 sqrt(2) qm each way, det_sincosf is within SINCOS_ABS of the float64 sine and cosine, and the
  nine products and sums that form an entry act on values of at most 2 qm:
      e_R = 8 (SINCOS_ABS + 2 u) qm        (per entry).
  It moves det S by at most (S_xx + S_yy + 2 |S_xy|) e_R <= 4 lambda_max(S) e_R, i.e. by rho = 4 e_R / lambda_min(S) of itself,
  and what follows is first order in e_R with the factor g = 1 / (1 - rho) for the rest.

  mean        |mu' - mu'_64| <= a_P e_d + 2 u (|t| + |mu| + |d|) + u (6 kappa(S) + 18) qm D / lambda_min(S)
                                + 2 g e_R D (1 + qm / lambda_min(S)) / lambda_min(S),
                  e_d = 4 u (|t| + |mu| + |d|) + 4 (SINCOS_ABS + u) |z|   (the error of w and of d, as in the isotropic bound),
                  D = |d| + e_d   (the innovation the arithmetic really sees),      a_P = max(1, ||P S^-1||_2).
              mu' = w - R S^-1 d = P S^-1 w + R S^-1 mu: an error dw of the observed point reaches the mean through P S^-1.  With
              Q = q I that matrix is symmetric with eigenvalues below 1 and the isotropic bound says 1; with an elongated Q across
              an elongated P it is far from normal and its norm is not bounded by 1 (up to sqrt(kappa(P) kappa(Q)) or so): at |pose|
              = 1e3 and P ~ 1e-8 the innovation is all rounding, and a bound without a_P is missed by 1.4 in the regime lambda_max(Q)
              = 1e-8, ratio 1e4, P / q = 1, kappa(P) = 1e4 — a property of the problem (the float64 sensitivity), not of the
              formula.  Where Q = q I (ratio 1) the test also asserts a_P = 1 and hence the bound without the factor.  The rest: the last subtraction; the roundings of S (u lambda_max(S) per entry), of det S and its reciprocal
              ((2 kappa(S) + 2) u), of S^-1 d and R (S^-1 d), and of d = w - mu, all through ||R|| ||S^-1|| <= qm / lambda_min(S);
              delta(R S^-1 d) = dR S^-1 d - R S^-1 dR S^-1 d with |dR| <= 2 e_R in norm.
  covariance  max |P'_ij - P'_64,ij| <= 4 u ((kappa(S) + 2) lambda_max(P') + qm (P_xx P_yy + P_xy^2) / det S)
                                + 4 u (qxx qyy + qxy^2) lambda_max(P) / det S
                                + g e_R (det P / det S + 4 lambda_max(P') / lambda_min(S))
              (isotropic bound with qm; the rounding of detq = qxx qyy - qxy^2, which multiplies P / det S; P' = N / D with
               N = det P R_w + det Q P, D = det S: dN = det P dR, dD <= 4 lambda_max(S) e_R)
  log-lik     |ll - ll_64| <= 8 u (kappa(S) (1 + m) + |log det S| + 1) + 2 sqrt(m / lambda_min(S)) e_d
                                + g e_R (m + 2) / lambda_min(S),      e_d = 4 u (|t| + |mu| + |d|) + 4 (SINCOS_ABS + u) |z|
              (delta(d^T S^-1 d) = -d^T S^-1 dR S^-1 d <= 2 e_R m / lambda_min(S); delta(log det S) <= rho)
  first sighting: the mean within 4 u (|t| + |w|) + 4 (SINCOS_ABS + u) |z| of w, every entry of P within e_R of R_w.
"""
import numpy as np
import pytest

import _aniso_spec as A
import _f64_pf as F

U, SC = F.U, F.SINCOS_ABS
N, REG = 4096, sorted({(r, k) for _, r, k in F.GRID})      # the 15 (P / q, kappa(P)) regimes of the grid
LC = 36                                                     # landmarks per regime: L = 540


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


def check(rows, out, ll, pose, zx, zy, cov, label, groups=None, normal=False):
    """One frame with every landmark observed: `out` / `ll` (the spec's, or anything that claims to implement it) against the
    reference and its bounds.  groups: {name: columns}, for the per-regime print.  normal: Q = q I, where P S^-1 is symmetric with
    eigenvalues below 1 — the mean must then meet the bound WITHOUT the factor a_P (a_P = 1): the factor loosens nothing
    there.  -> worst ratios over the frame."""
    n, _, L = rows.shape
    p, g = np.moveaxis(rows, 1, 0), np.moveaxis(out, 1, 0)
    first = p[2] < 0
    seen = ~first
    x, y, th = (np.asarray(a)[:, None] for a in pose)
    pp = np.where(seen, p, np.array([0, 0, 1, 0, 1], np.float32)[:, None, None])
    ref, b = bounds(pp, (x, y, th), zx[None], zy[None], cov)
    r_mean = np.where(seen, np.hypot(g[0] - ref[0], g[1] - ref[1]) / b["mean"], 0.0)
    e_cov = np.maximum(np.maximum(np.abs(g[2] - ref[2]), np.abs(g[3] - ref[3])), np.abs(g[4] - ref[4]))
    r_cov = np.where(seen, e_cov / b["cov"], 0.0)
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


def regimes_frame(rng, q):
    """n x 540: landmark l is in regime l mod 15 of the grid at this q (P's largest eigenvalue r q, condition number k), every
    landmark observed, |pose| up to 1e3, 10 % of the pairs not seen yet."""
    L = LC * len(REG)
    rows, zx, zy = np.empty((N, 5, L), np.float32), np.empty(L, np.float32), np.empty(L, np.float32)
    pose, groups = None, {}
    for j, (r, k) in enumerate(REG):
        cols = np.arange(j, L, len(REG))
        pose, rows[:, :, cols], zx[cols], zy[cols] = F.regime_frame(rng, N, LC, q, r, k, pose=pose)
        groups[f"P/q={r:g} kappa={k:g}"] = cols
    rows[:, 2][rng.random((N, L)) < 0.1] = -1.0
    return pose, rows, zx, zy, groups


@pytest.mark.parametrize("ratio", [1.0, 1e2, 1e4])
@pytest.mark.parametrize("q", sorted({q for q, _, _ in F.GRID}))
def test_spec_within_its_bounds_of_the_float64_ekf(orc, q, ratio):
    rng = np.random.default_rng(int(1e9 * q) + int(ratio))
    cov = q_matrix(q, ratio, rng.uniform(0, np.pi))
    pose, rows, zx, zy, groups = regimes_frame(rng, q)
    out, ll = A.update(rows, *pose, None, np.arange(rows.shape[2]), zx, zy, cov)
    check(rows, out, ll, pose, zx, zy, cov, f"lambda_max(Q)={q:g} ratio={ratio:g}", groups, normal=ratio == 1.0)


def test_isotropic_q_agrees_with_the_isotropic_oracle(orc):
    """Q = q I: the spec and orc_ekf_update both lie within the float64 bounds of the same reference (bit equality is not claimed:
    the operation orders differ)."""
    rng = np.random.default_rng(3)
    q = 1e-2
    pose, rows, zx, zy, _ = regimes_frame(rng, q)
    cov = (np.float32(q), np.float32(0.0), np.float32(q))
    ids = np.arange(rows.shape[2])
    out, ll = A.update(rows, *pose, None, ids, zx, zy, cov)
    check(rows, out, ll, pose, zx, zy, cov, "spec, Q = q I", normal=True)
    out_iso, ll_iso = orc.ekf_update(rows, *pose, None, ids.astype(np.int32), zx, zy, float(np.float32(q)))
    check(rows, out_iso, ll_iso, pose, zx, zy, cov, "orc_ekf_update")
    print(f"spec vs orc_ekf_update: rows equal bit for bit on {np.mean(out.view(np.uint32) == out_iso.view(np.uint32)):.3f} of the values")


def test_k_sightings_of_a_static_point_give_r_w_over_k(orc):
    """A point seen k times from one pose: P = R_w / k.  Each step's error is within its covariance bound and an earlier error is
    passed on through P S^-1 = (j - 1) / j I, a contraction: the bounds add up."""
    rng = np.random.default_rng(4)
    n, k = 512, 12
    cov = q_matrix(4e-2, 1e2, 0.7)
    x, y, th = (rng.uniform(-100, 100, n).astype(np.float32) for _ in range(3))
    zx, zy = np.array([3.0], np.float32), np.array([-1.5], np.float32)
    rows = np.zeros((n, 5, 1), np.float32)
    rows[:, 2] = -1.0
    rw = world_noise64(cov, th)
    budget = np.zeros(n)
    for j in range(1, k + 1):
        prior = rows
        rows, _ = A.update(rows, x, y, th, None, [0], zx, zy, cov)
        if j == 1:
            budget += 8.0 * (SC + 2 * U) * float(max(cov[0], cov[2]))
        else:
            _, b = bounds(np.moveaxis(prior, 1, 0), (x[:, None], y[:, None], th[:, None]), zx[None], zy[None], cov)
            budget += b["cov"][:, 0]
        err = np.max([np.abs(rows[:, 2 + i, 0] - rw[i] / j) for i in range(3)], axis=0)
        assert np.all(err <= budget), f"sighting {j}: {np.max(err / budget):.3g} x the accumulated bound"
    print(f"{k} sightings: max |P - R_w / k| / accumulated bound {np.max(err / budget):.3g}")


def test_the_mean_converges_faster_along_the_small_axis(orc):
    """A landmark whose prior mean is off by the same amount along both sensor axes, prior P = p I with lambda_min(Q) < p <
    lambda_max(Q): one exact observation takes q / (p + q) of the offset away along each axis — most of it along the small one."""
    rng = np.random.default_rng(5)
    n = 1024
    q_small, q_large, p0, off = 1e-4, 1.0, 1e-2, 0.05
    cov = (np.float32(q_small), np.float32(0.0), np.float32(q_large))          # sensor x: the accurate axis
    x, y, th = (rng.uniform(-20, 20, n).astype(np.float32) for _ in range(3))
    zx, zy = np.array([4.0], np.float32), np.array([2.0], np.float32)
    c, s = np.cos(th.astype(np.float64)), np.sin(th.astype(np.float64))
    wx, wy = F.first_sighting(zx, zy, x, y, th)                               # the true point, per particle
    # the offset in the world frame: H^T (off, off)
    rows = np.zeros((n, 5, 1), np.float32)
    rows[:, 0, 0] = wx + (c * off + s * off)
    rows[:, 1, 0] = wy + (-s * off + c * off)
    rows[:, 2, 0] = rows[:, 4, 0] = p0
    out, _ = A.update(rows, x, y, th, None, [0], zx, zy, cov)
    ex, ey = out[:, 0, 0].astype(np.float64) - wx, out[:, 1, 0].astype(np.float64) - wy
    left_small, left_large = c * ex - s * ey, s * ex + c * ey                  # back in the sensor frame: H e
    assert np.all(np.abs(left_small) < 0.1 * np.abs(left_large))
    assert np.allclose(left_large, off * q_large / (p0 + q_large), rtol=1e-3, atol=1e-5)
    assert np.all(np.abs(left_small) < off * q_small / (p0 + q_small) + 1e-4)
    print(f"offset left along the small / large axis: {np.abs(left_small).max():.2e} / {np.abs(left_large).min():.2e} of {off}")
