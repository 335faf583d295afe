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
from _aniso_bounds import bounds, check, ekf64, q_matrix, world_noise64   # noqa: F401 - the one copy; other tests import them from here

U, SC = F.U, F.SINCOS_ABS
N, REG = 4096, sorted({(r, k) for _, r, k in F.GRID})      # the 15 (P / q, kappa(P)) regimes of the grid
LC = 36                                                     # landmarks per regime: L = 540


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
