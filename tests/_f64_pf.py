"""An independent float64 reference of the particle-filter stages (motion sample, landmark EKF, weights, resample).

It imports neither `oracle` nor the package, and it does not use the world-frame algebra of the specification
(csrc/ekf_math.h, oracle/slam_oracle_pf.c): the landmark update is the textbook one in the SENSOR frame,
    H = [[c, -s], [s, c]],  v = z - H (mu - t),  S = H P H^T + q I,  K = P H^T S^-1,
    mu' = mu + K v,  P' = (I - K H) P (I - K H)^T + q K K^T  (Joseph form),
    ll = -1/2 v^T S^-1 v - 1/2 log det S - log 2 pi,
with every 2 x 2 product written out and evaluated in float64 on whole arrays.  What the specification's float32
arithmetic is measured against, and what tests/test_pf_f64_spec.py and tests/test_gpu_pf_f64.py bound its error by.
"""
import numpy as np

U32 = np.uint64(0xFFFFFFFF)
LOG_2PI = np.log(2.0 * np.pi)


def philox4x32_10(ctr, key):
    """Philox4x32-10 (Salmon et al., SC'11) on arrays: ctr = 4 arrays of uint32 counters, key = 2 ints -> 4 uint64 arrays."""
    c = [np.asarray(v, np.uint64) & U32 for v in ctr]
    k0, k1 = np.uint64(key[0] & 0xFFFFFFFF), np.uint64(key[1] & 0xFFFFFFFF)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & U32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & U32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return c


def motion_noise(n, first_id, seed, frame):
    """The standard normals (z0, z1, z2) of slots first_id .. first_id + n - 1: Box-Muller in float64 on the 24-bit
    uniforms of the motion stream (counter = slot id lo, hi, frame, 0)."""
    gid = np.arange(first_id, first_id + n, dtype=np.uint64)
    zero = np.zeros(n, np.uint64)
    r = philox4x32_10([gid & U32, gid >> np.uint64(32), zero + np.uint64(frame), zero], (seed, seed >> 32))
    u = [(r[k] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24 for k in range(4)]
    u1, u3 = u[0] + 2.0 ** -24, u[2] + 2.0 ** -24          # (0, 1] for the radii, [0, 1) for the angles
    rad1, rad2 = np.sqrt(-2.0 * np.log(u1)), np.sqrt(-2.0 * np.log(u3))
    return rad1 * np.cos(2 * np.pi * u[1]), rad1 * np.sin(2 * np.pi * u[1]), rad2 * np.cos(2 * np.pi * u[3])


def motion_sample(src, anc, first_id, dp, sigma, seed, frame):
    """src: [3][n_src] poses; anc: ancestor of every slot (None: the identity) -> [3][n] float64 poses, and the noise."""
    src = np.asarray(src, np.float64)
    n = src.shape[1] if anc is None else len(anc)
    j = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    z = motion_noise(n, first_id, seed, frame)
    out = np.stack([src[k, j] + float(np.float32(dp[k])) + float(np.float32(sigma[k])) * z[k] for k in range(3)])
    return out, np.stack(z)


def ekf_update(mx, my, pxx, pxy, pyy, zx, zy, px, py, th, q):
    """One landmark update per element (all arrays broadcast together; float64).  Landmarks seen before only.
    Returns (mu_x', mu_y', P_xx', P_xy', P_yy', ll) and the diagnostics the error bounds need: S (s00, s01, s11), the
    innovation v and t = the pose."""
    f = lambda a: np.asarray(a, np.float64)
    mx, my, pxx, pxy, pyy, zx, zy, px, py, th = map(f, (mx, my, pxx, pxy, pyy, zx, zy, px, py, th))
    q = float(q)
    c, s = np.cos(th), np.sin(th)
    h00, h01, h10, h11 = c, -s, s, c
    ex, ey = mx - px, my - py
    vx = zx - (h00 * ex + h01 * ey)
    vy = zy - (h10 * ex + h11 * ey)
    # A = H P, S = A H^T + q I
    a00, a01 = h00 * pxx + h01 * pxy, h00 * pxy + h01 * pyy
    a10, a11 = h10 * pxx + h11 * pxy, h10 * pxy + h11 * pyy
    s00 = a00 * h00 + a01 * h01 + q
    s01 = a00 * h10 + a01 * h11
    s11 = a10 * h10 + a11 * h11 + q
    dS = s00 * s11 - s01 * s01
    j00, j01, j11 = s11 / dS, -s01 / dS, s00 / dS
    # B = P H^T = A^T, K = B S^-1
    k00, k01 = a00 * j00 + a10 * j01, a00 * j01 + a10 * j11
    k10, k11 = a01 * j00 + a11 * j01, a01 * j01 + a11 * j11
    mux = mx + (k00 * vx + k01 * vy)
    muy = my + (k10 * vx + k11 * vy)
    # M = I - K H, P' = M P M^T + q K K^T
    m00 = 1.0 - (k00 * h00 + k01 * h10)
    m01 = -(k00 * h01 + k01 * h11)
    m10 = -(k10 * h00 + k11 * h10)
    m11 = 1.0 - (k10 * h01 + k11 * h11)
    b00, b01 = m00 * pxx + m01 * pxy, m00 * pxy + m01 * pyy
    b10, b11 = m10 * pxx + m11 * pxy, m10 * pxy + m11 * pyy
    o2 = b00 * m00 + b01 * m01 + q * (k00 * k00 + k01 * k01)
    o3 = b00 * m10 + b01 * m11 + q * (k00 * k10 + k01 * k11)
    o4 = b10 * m10 + b11 * m11 + q * (k10 * k10 + k11 * k11)
    maha = vx * (j00 * vx + j01 * vy) + vy * (j01 * vx + j11 * vy)
    ll = -0.5 * maha - 0.5 * np.log(dS) - LOG_2PI
    return (mux, muy, o2, o3, o4, ll), {"s00": s00, "s01": s01, "s11": s11, "vx": vx, "vy": vy, "maha": maha}


def first_sighting(zx, zy, px, py, th):
    """The observed point in the world frame, t + H^T z (what a first sighting stores; P = q I)."""
    c, s = np.cos(np.asarray(th, np.float64)), np.sin(np.asarray(th, np.float64))
    zx, zy = np.asarray(zx, np.float64), np.asarray(zy, np.float64)
    return np.asarray(px, np.float64) + (c * zx + s * zy), np.asarray(py, np.float64) + (-s * zx + c * zy)


def update_rows(prior, pose, ids, zx, zy, q, L):
    """Whole landmark rows: prior [n][5][>= L] float32, pose [3][n], observations (ids unique, any order).
    -> (rows [n][5][L] float64, loglik [n] float64, per-landmark ll [n][k] float64, mask of first sightings [n][k]).
    Unobserved landmarks keep their prior; a prior P_xx < 0 marks a landmark never seen (first sighting: mu = t + H^T z,
    P = q I, no likelihood term)."""
    prior = np.asarray(prior)
    out = prior[:, :, :L].astype(np.float64)
    ids = np.asarray(ids, np.int64)
    n = prior.shape[0]
    if len(ids) == 0:
        return out, np.zeros(n), np.zeros((n, 0)), np.zeros((n, 0), bool)
    p = prior[:, :, ids].astype(np.float64)                                     # [n][5][k]
    x, y, th = (np.asarray(pose[k], np.float64)[:, None] for k in range(3))
    zx, zy = np.asarray(zx, np.float64)[None, :], np.asarray(zy, np.float64)[None, :]
    first = p[:, 2] < 0
    pxx = np.where(first, 1.0, p[:, 2])
    (o0, o1, o2, o3, o4, ll), _ = ekf_update(p[:, 0], p[:, 1], pxx, np.where(first, 0.0, p[:, 3]),
                                             np.where(first, 1.0, p[:, 4]), zx, zy, x, y, th, q)
    fx, fy = first_sighting(zx, zy, x, y, th)
    qf = float(np.float32(q))
    out[:, 0, ids] = np.where(first, fx, o0)
    out[:, 1, ids] = np.where(first, fy, o1)
    out[:, 2, ids] = np.where(first, qf, o2)
    out[:, 3, ids] = np.where(first, 0.0, o3)
    out[:, 4, ids] = np.where(first, qf, o4)
    ll = np.where(first, 0.0, ll)
    return out, ll.sum(axis=1), ll, first


def logweights(loglik, score, gain):
    return np.asarray(loglik, np.float64) - float(np.float32(gain)) * np.asarray(score, np.float64)


def weights(logw):
    """exp(logw - max) and the quantised weights the resample works on, w * 2^32 (float64, not truncated)."""
    lw = np.asarray(logw, np.float64)
    w = np.exp(lw - lw.max())
    return w, w * 4294967296.0


def comb_offset(seed, frame, total):
    """The comb's offset u in [0, total) of frame `frame`: Philox counter (0, 0, frame, 1), u = floor(r64 * total / 2^64)."""
    r = philox4x32_10([np.uint64(0), np.uint64(0), np.uint64(frame), np.uint64(1)], (seed, seed >> 32))
    r64 = int(r[0]) | (int(r[1]) << 32)
    return (r64 * int(total)) >> 64


def resample(w, tooth):
    """Systematic resampling in float64: slot j goes to the particle whose normalised CDF interval holds (j + tooth) / n.
    w: weights (any scale); tooth in [0, 1).  -> (ancestors [n], the normalised CDF [n], the tooth positions [n])."""
    w = np.asarray(w, np.float64)
    n = len(w)
    cdf = np.cumsum(w) / w.sum()
    pos = (np.arange(n) + tooth) / n
    anc = np.minimum(np.searchsorted(cdf, pos, side="right"), n - 1)
    return anc, cdf, pos


# ---------------------------------------------------------------- the regime grid and the forward-error bounds
U = 2.0 ** -24                    # unit roundoff of float32
SINCOS_ABS = 2.6e-7               # det_sincosf's absolute error for |theta| <= 2e4

# (q, P / q, kappa(P)): the measurement variance, the prior's largest eigenvalue over q and its condition number
GRID = [(q, r, k) for q in (1e-8, 1e-4, 1e-2) for r in (1e-4, 1.0, 1e2, 1e4, 1e8) for k in (1.0, 1e2, 1e4)]


def random_priors(rng, shape, q, ratio, kappa):
    """Covariances with eigenvalues (ratio q, ratio q / kappa) at uniformly random orientations, as float32."""
    lam1 = ratio * q
    lam2 = lam1 / kappa
    phi = rng.uniform(0, np.pi, shape)
    c, s = np.cos(phi), np.sin(phi)
    pxx = lam1 * c * c + lam2 * s * s
    pxy = (lam1 - lam2) * c * s
    pyy = lam1 * s * s + lam2 * c * c
    return pxx.astype(np.float32), pxy.astype(np.float32), pyy.astype(np.float32)


def regime_frame(rng, n, L, q, ratio, kappa, pose_max=1e3, theta_max=1e3, range_max=1e3, huge_every=0, pose=None):
    """One frame of the regime, every landmark observed: poses (|x|, |y| <= pose_max, |theta| <= theta_max), prior rows
    [n][5][L] float32 with the regime's covariances, and one observation (zx, zy) per landmark, up to range_max from the
    pose.  Each particle's prior mean is the point it observes displaced by a draw from its own covariance, so that the
    innovation is typical (|d| ~ sqrt(lambda(P))).
    huge_every = k > 0: on every k-th particle about half the covariances are ~1e10 m^2 (det (P + q I) beyond 2^61: the
    division fallback of the device reciprocal, mixed with ordinary lanes in the same wavefronts)."""
    if pose is None:
        pose = (rng.uniform(-pose_max, pose_max, n).astype(np.float32), rng.uniform(-pose_max, pose_max, n).astype(np.float32),
                rng.uniform(-theta_max, theta_max, n).astype(np.float32))
    x, y, th = pose
    pxx, pxy, pyy = random_priors(rng, (n, L), q, ratio, kappa)
    if huge_every:
        hx, hxy, hy = random_priors(rng, (n, L), 1.0, 1e10, 10.0)
        sel = (np.arange(n) % huge_every == 0)[:, None] & (rng.random((n, L)) < 0.5)
        pxx, pxy, pyy = np.where(sel, hx, pxx), np.where(sel, hxy, pxy), np.where(sel, hy, pyy)
    # the observations, common to all particles; the landmark each particle observes is t + H^T z (from its own pose)
    ang = rng.uniform(-np.pi, np.pi, L)
    rad = range_max * np.sqrt(rng.uniform(0.0, 1.0, L))
    zx = (rad * np.cos(ang)).astype(np.float32)
    zy = (rad * np.sin(ang)).astype(np.float32)
    wx, wy = first_sighting(zx[None, :], zy[None, :], x[:, None], y[:, None], th[:, None])
    g = rng.standard_normal((2, n, L))
    p64 = [a.astype(np.float64) for a in (pxx, pxy, pyy)]
    l00 = np.sqrt(p64[0])
    l10 = p64[1] / np.where(l00 > 0, l00, 1.0)
    l11 = np.sqrt(np.maximum(p64[2] - l10 * l10, 0.0))
    rows = np.empty((n, 5, L), np.float32)
    rows[:, 0] = wx + l00 * g[0]
    rows[:, 1] = wy + l10 * g[0] + l11 * g[1]
    rows[:, 2], rows[:, 3], rows[:, 4] = pxx, pxy, pyy
    return (x, y, th), rows, zx, zy


def mixed_frame(rng, n, L, q, pose=None, huge=True, first_frac=0.1, **kw):
    """regime_frame with the regime changing from landmark to landmark: landmark l takes the grid's (P / q, kappa(P)) number
    l mod 15 (at this q), every 16th landmark a ~1e10 m^2 prior on half the particles (huge), and a fraction first_frac of
    the (particle, landmark) pairs not seen yet (P_xx = -1)."""
    regimes = [(r, k) for qq, r, k in GRID if qq == GRID[0][0]]
    rows = np.empty((n, 5, L), np.float32)
    zx, zy = np.empty(L, np.float32), np.empty(L, np.float32)
    for j, (r, k) in enumerate(regimes):
        cols = np.arange(j, L, len(regimes) + 1)
        if len(cols) == 0:
            continue
        pose, rows[:, :, cols], zx[cols], zy[cols] = regime_frame(rng, n, len(cols), q, r, k, pose=pose, **kw)
    cols = np.arange(len(regimes), L, len(regimes) + 1)
    if len(cols):
        pose, rows[:, :, cols], zx[cols], zy[cols] = regime_frame(rng, n, len(cols), q, 1e2, 1.0, pose=pose,
                                                                  huge_every=2 if huge else 0, **kw)
    rows[:, 2][rng.random((n, L)) < first_frac] = -1.0
    return pose, rows, zx, zy


def motion_errors(got, src, anc, dp, sigma, first_id, seed, frame):
    """(error / bound) of float32 motion samples got [3][n] against the float64 Box-Muller reference.  The bound:
    |x - x_64| <= 4 u (|x_src| + |dp|) + 40 u sigma R, R = sqrt(-2 log 2^-24) the largest Box-Muller radius (det_logf and
    det_sincosf each within a few u, the float32 2 pi within u)."""
    want, _ = motion_sample(src, anc, first_id, dp, sigma, seed, frame)
    j = np.arange(want.shape[1]) if anc is None else np.asarray(anc)
    r_max = np.sqrt(-2.0 * np.log(2.0 ** -24))
    out = []
    for k in range(3):
        b = 4 * U * (np.abs(np.asarray(src[k], np.float64)[j]) + abs(float(np.float32(dp[k])))) + 40 * U * float(np.float32(sigma[k])) * r_max
        out.append(np.abs(np.asarray(got[k], np.float64) - want[k]) / b)
    return np.stack(out)


def _eig2(a, b, c):
    """eigenvalues (small, large) of the symmetric [[a, b], [b, c]] (float64 arrays)"""
    m, d = 0.5 * (a + c), np.hypot(0.5 * (a - c), b)
    hi = m + d
    det = a * c - b * b
    return det / hi, hi


def update_errors(got, prior, pose, zx, zy, q):
    """Errors of float32 landmark updates `got` (posterior [5][...]) against the float64 reference, each over its
    forward-error bound (a ratio <= 1 is within the bound).  prior [5][...], pose (x, y, theta) and z broadcast with it.
    The bounds (u = 2^-24; kappa(S) with S = P + q I; lambda_min(S); d the innovation; w = t + H^T z):
      mean        |mu' - mu'_64|  <= 4 u (|t| + |mu| + |d| (1 + kappa(S) q / lambda_min(S))) + 4 (SINCOS_ABS + u) |z|
      covariance  max |P'_ij - P'_64,ij| <= 4 u ((kappa(S) + 2) lambda_max(P') + q (P_xx P_yy + P_xy^2) / det S)
      log-lik     |ll - ll_64| <= 8 u (kappa(S) (1 + m) + |log det S| + 1) + 2 sqrt(m / lambda_min(S)) e_d,
                  m = d^T S^-1 d,  e_d = 4 u (|t| + |mu| + |d|) + 4 (SINCOS_ABS + u) |z|   (the error of d itself)
    Positive definiteness of the stored P' is returned separately (exact, in float64 from the float32 values)."""
    p = [np.asarray(a, np.float64) for a in prior]
    g = [np.asarray(a, np.float64) for a in got[:5]]
    px, py, th = (np.asarray(a, np.float64) for a in pose)
    (r0, r1, r2, r3, r4, rll), dg = ekf_update(p[0], p[1], p[2], p[3], p[4], zx, zy, px, py, th, q)
    q = float(q)
    lmin_s, lmax_s = _eig2(dg["s00"], dg["s01"], dg["s11"])
    lmin_p, lmax_p = _eig2(p[2], p[3], p[4])
    kap_s = lmax_s / lmin_s
    kap_p = lmax_p / np.maximum(lmin_p, lmax_p * 1e-30)
    t = np.hypot(px, py)
    mu = np.hypot(p[0], p[1])
    d = np.hypot(dg["vx"], dg["vy"])
    z = np.hypot(np.asarray(zx, np.float64), np.asarray(zy, np.float64))
    sc = 4.0 * (SINCOS_ABS + U) * z
    b_mean = 4 * U * (t + mu + d * (1.0 + kap_s * q / lmin_s)) + sc
    e_mean = np.hypot(g[0] - r0, g[1] - r1)
    _, lmax_post = _eig2(r2, r3, r4)
    b_cov = 4 * U * ((kap_s + 2.0) * lmax_post + q * (p[2] * p[4] + p[3] * p[3]) / (lmin_s * lmax_s))
    e_cov = np.maximum(np.maximum(np.abs(g[2] - r2), np.abs(g[3] - r3)), np.abs(g[4] - r4))
    pd = (g[2] > 0) & (g[4] > 0) & (g[2] * g[4] - g[3] * g[3] > 0)
    m = dg["maha"]
    e_d = 4 * U * (t + mu + d) + sc
    b_ll = 8 * U * (kap_s * (1.0 + m) + np.abs(np.log(lmin_s * lmax_s)) + 1.0) + 2.0 * np.sqrt(m / lmin_s) * e_d
    out = {"mean": e_mean / b_mean, "cov": e_cov / b_cov, "pd": pd, "ll_ref": rll, "b_ll": b_ll}
    if len(got) > 5:
        out["ll"] = np.abs(np.asarray(got[5], np.float64) - rll) / b_ll
    return out


def resample_check(wq_dev, anc_dev, logw, seed, frame, total_dev=None):
    """Ancestors of a systematic resample from quantised weights against the float64 resample of the same log-weights.
    The quantised weight of particle i is within e_i = w64_i (6 u + 2 u |logw_i - max|) + 1 of w64_i = exp(logw_i - max) 2^32
    (det_expf: 3e-7 relative; the rounding of logw - max; the truncation), so the device's normalised CDF is within
    (E_i + E_n) / T of the float64 one (E_i = e_0 + .. + e_i, T = the float64 total) and its comb tooth within 1 / T of
    u / total.  A slot may have another ancestor than the float64 resample gives only if its tooth lies within that error
    of every CDF boundary between the two ancestors; no particle's offspring count may differ by more than 1.
    wq_dev None: the device's total is not known, and the float64 total is used (its error is added to every tooth's).
    Returns (slots that differ, largest count difference); raises AssertionError on a difference that is not explained."""
    lw = np.asarray(logw, np.float64)
    n = len(lw)
    _, w64 = weights(lw)
    T = w64.sum()
    e = w64 * (6 * U + 2 * U * np.abs(lw - lw.max())) + 1.0
    E = np.cumsum(e)
    tol = (E + E[-1]) / T + 2.0 / (n * T) + 1e-15
    if total_dev is None and wq_dev is not None:
        total_dev = int(np.asarray(wq_dev, np.uint64).sum())
    if total_dev is None:   # the device's total is not known: the float64 one, and its error on every tooth
        total_dev = int(round(T))
        tol = tol + E[-1] / T
    tooth = comb_offset(seed, frame, total_dev) / total_dev
    anc64, cdf, pos = resample(w64, tooth)
    anc_dev = np.asarray(anc_dev, np.int64)
    diff = np.nonzero(anc_dev != anc64)[0]
    for j in diff:
        lo, hi = sorted((int(anc_dev[j]), int(anc64[j])))
        near = np.abs(pos[j] - cdf[lo:hi]) <= tol[lo:hi]
        assert near.all(), (f"slot {j}: ancestor {anc_dev[j]}, float64 {anc64[j]}; tooth {pos[j]!r} is "
                            f"{np.abs(pos[j] - cdf[lo:hi]).max():.3g} from a CDF boundary, allowed {tol[lo:hi].min():.3g}")
    dc = np.abs(np.bincount(anc_dev, minlength=n) - np.bincount(anc64, minlength=n)).max() if n else 0
    assert dc <= 1, f"offspring counts differ by {dc}"
    return len(diff), int(dc)


def check_frame(rows, out, ll, pose, ids, zx, zy, q, label, L=None):
    """One frame of landmark updates: prior rows [n][5][Lp >= L] float32, the updated rows `out` and log-likelihoods `ll` (the
    specification's or a kernel's), poses (x, y, theta) [n], the observations (ids in any order, zx / zy in that order).
    Every quantity against the float64 reference and its bound (update_errors); first sightings placed at the observed
    point with P = q I exactly; unobserved landmarks untouched; every posterior positive definite.  Prints and returns
    the worst error / bound ratios."""
    L = rows.shape[2] if L is None else L            # rows may be padded beyond L
    rows, out = rows[:, :, :L], out[:, :, :L]
    ids = np.asarray(ids)
    p = np.moveaxis(rows[:, :, ids], 1, 0)                 # [5][n][k]
    g = np.moveaxis(out[:, :, ids], 1, 0)
    first = p[2] < 0
    seen = ~first
    x, y, th = (np.asarray(a)[:, None] for a in pose)
    pp = np.where(seen, p, np.array([0, 0, 1, 0, 1], np.float32)[:, None, None])
    zxo, zyo = np.asarray(zx)[None], np.asarray(zy)[None]   # one observation per id, in the order of ids
    r = update_errors(g, pp, (x, y, th), zxo, zyo, q)
    worst = {"mean": float(np.max(r["mean"][seen], initial=0)), "cov": float(np.max(r["cov"][seen], initial=0))}
    # posterior covariance positive definite, exactly (float64 from the stored float32 values)
    npd = int((~r["pd"][seen]).sum())
    # first sightings: the observed point (the mean bound's w-terms), P = q I exactly
    fx, fy = first_sighting(zxo, zyo, x, y, th)
    b_first = 4 * U * np.hypot(x, y) + 4 * (SINCOS_ABS + U) * np.hypot(zxo, zyo) + 4 * U * np.hypot(fx, fy)
    e_first = np.hypot(g[0] - fx, g[1] - fy) / b_first
    worst["first"] = float(np.max(e_first[first], initial=0))
    qf = np.float32(q)
    assert (g[2][first] == qf).all() and (g[3][first] == 0).all() and (g[4][first] == qf).all(), f"{label}: first P != q I"
    # unobserved landmarks: untouched
    rest = np.setdiff1d(np.arange(L), ids)
    assert np.array_equal(out[:, :, rest].view(np.uint32), rows[:, :, rest].view(np.uint32)), f"{label}: unobserved changed"
    # the log-likelihood sum over landmarks
    ll64 = np.where(seen, r["ll_ref"], 0.0)
    b_sum = np.where(seen, r["b_ll"], 0.0).sum(axis=1) + (-(-L // 128) + 7) * U * np.abs(ll64).sum(axis=1) + 1e-30
    worst["loglik"] = float((np.abs(np.asarray(ll, np.float64) - ll64.sum(axis=1)) / b_sum).max())
    print(f"{label}: max error / bound  mean {worst['mean']:.3g}  cov {worst['cov']:.3g}  first {worst['first']:.3g}  "
          f"loglik {worst['loglik']:.3g}; non-positive-definite posteriors {npd}")
    for k, v in worst.items():
        assert v <= 1.0, f"{label}: {k} error {v:.3g} x its bound"
    assert npd == 0, f"{label}: {npd} posteriors not positive definite"
    return worst
