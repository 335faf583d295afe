"""The float64 sensor-frame Mahalanobis term of a (landmark, detection) pair under a 2x2 measurement covariance and the bound on
the specification's world-frame cost.  TEST INFRASTRUCTURE shared by test_assoc_aniso_spec_cpu.py (whose docstring holds the
derivation) and the regime tests: one copy of the formula.  numpy and _f64_pf only."""
import numpy as np

import _f64_pf as F

U, SC = F.U, F.SINCOS_ABS


def cost64(rows, x, y, th, zx, zy, cov):
    """m_64 [n][L][K] in the sensor frame and what the bound needs."""
    f = lambda a: np.asarray(a, np.float64)
    mx, my, pxx, pxy, pyy = (f(rows[:, j])[:, :, None] for j in range(5))
    px, py, t = (f(a)[:, None, None] for a in (x, y, th))
    zx, zy = f(zx)[None, None, :], f(zy)[None, None, :]
    qxx, qxy, qyy = (float(v) for v in cov)
    c, s = np.cos(t), np.sin(t)
    ex, ey = mx - px, my - py
    vx = zx - (c * ex - s * ey)                                    # H = [[c, -s], [s, c]]
    vy = zy - (s * ex + c * ey)
    a00, a01 = c * pxx - s * pxy, c * pxy - s * pyy                # H P
    a10, a11 = s * pxx + c * pxy, s * pxy + c * pyy
    s00 = a00 * c - a01 * s + qxx                                  # H P H^T + Q
    s01 = a00 * s + a01 * c + qxy
    s11 = a10 * s + a11 * c + qyy
    det = s00 * s11 - s01 * s01
    m = (vx * (s11 * vx - s01 * vy) + vy * (s00 * vy - s01 * vx)) / det
    lmin, lmax = F._eig2(s00, s01, s11)
    _, qm = F._eig2(np.float64(qxx), np.float64(qxy), np.float64(qyy))
    tn, mu, d, z = np.hypot(px, py), np.hypot(mx, my), np.hypot(vx, vy), np.hypot(zx, zy)
    e_d = 4 * U * (tn + mu + d) + 4 * (SC + U) * z
    big_d = 2 * np.sqrt(m / lmin) * e_d + e_d * e_d / lmin
    e_s = U * lmax + 8.0 * (SC + 2 * U) * qm
    g = 1.0 / (1.0 - 2 * e_s / lmin)
    assert np.all(g > 0)
    kap = lmax / lmin
    bound = big_d + (U * (5.5 * kap + 3.5) + 2 * g * e_s / lmin) * (m + big_d)
    return m, bound
