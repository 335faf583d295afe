"""The specification of the landmark update with a 2x2 sensor-frame measurement covariance ("General
measurement covariance"; include/slam_hip.h: slam_ekf_update_aniso_dev) in numpy float32, one rounded operation per line.
TEST INFRASTRUCTURE shared by test_aniso_spec_cpu.py and the GPU tests.  It uses the CPU oracle's deterministic sine / cosine
and logarithm and numpy's float32 division, and nothing of the package; the walk over a row and the order in which a
particle's log-likelihood terms are summed are those of oracle/slam_oracle_pf.c: orc_ekf_update.

Q = [[qxx, qxy], [qxy, qyy]] in the sensor frame, H^T = [[c, s], [-s, c]] with (s, c) = det_sincos(theta).
"""
import numpy as np

import oracle

F = np.float32
LANES = 128


def valid_cov(meas_cov):
    """What slam_ekf_update_aniso_dev accepts: finite, qxx > 0, qyy > 0, float32 determinant > 0."""
    q = np.asarray(meas_cov, np.float32)
    with np.errstate(all="ignore"):
        return bool(np.all(np.isfinite(q)) and q[0] > 0 and q[2] > 0 and det_q(q) > 0)


def det_q(meas_cov):
    """Once per session: detq = qxx*qyy - qxy*qxy in float32."""
    qxx, qxy, qyy = (F(v) for v in meas_cov)
    t0 = qxx * qyy
    t1 = qxy * qxy
    return F(t0 - t1)


def world_noise(meas_cov, s, c):
    """Once per particle: R_w = H^T Q H -> (rxx, rxy, ryy), float32 arrays like s and c."""
    qxx, qxy, qyy = (F(v) for v in meas_cov)
    s, c = np.asarray(s, np.float32), np.asarray(c, np.float32)
    t = c * qxx
    u = s * qxy
    a0 = t + u
    t = c * qxy
    u = s * qyy
    a1 = t + u
    t = c * qxy
    u = s * qxx
    b0 = t - u
    t = c * qyy
    u = s * qxy
    b1 = t - u
    t = a0 * c
    u = a1 * s
    rxx = t + u
    t = a1 * c
    u = a0 * s
    rxy = t - u
    t = b1 * c
    u = b0 * s
    ryy = t - u
    return rxx, rxy, ryy


def observed_point(zx, zy, s, c, px, py):
    """w = t + H^T z, exactly as ekf_particle / ekf_first_sighting."""
    t = c * zx
    u = s * zy
    t = t + u
    wx = px + t
    t = c * zy
    u = s * zx
    t = t - u
    wy = py + t
    return wx, wy


def update_one(mx, my, pxx, pxy, pyy, zx, zy, s, c, px, py, rxx, rxy, ryy, detq):
    """One landmark seen before, per element (float32 arrays that broadcast) -> (mu_x', mu_y', P_xx', P_xy', P_yy', ll)."""
    wx, wy = observed_point(zx, zy, s, c, px, py)
    dx = wx - mx
    dy = wy - my
    a = pxx + rxx
    b = pxy + rxy
    cc = pyy + ryy
    t = a * cc
    u = b * b
    det = t - u
    idet = F(1.0) / det
    i00 = cc * idet
    i01 = (-b) * idet
    i11 = a * idet
    t = i00 * dx
    u = i01 * dy
    t0 = t + u
    t = i01 * dx
    u = i11 * dy
    t1 = t + u
    t = rxx * t0
    u = rxy * t1
    t = t + u
    o0 = wx - t
    t = rxy * t0
    u = ryy * t1
    t = t + u
    o1 = wy - t
    t = pxx * pyy
    u = pxy * pxy
    detp = t - u
    t = detp * rxx
    u = detq * pxx
    t = t + u
    o2 = idet * t
    t = detp * rxy
    u = detq * pxy
    t = t + u
    o3 = idet * t
    t = detp * ryy
    u = detq * pyy
    t = t + u
    o4 = idet * t
    t = dx * t0
    u = dy * t1
    maha = t + u
    lg = oracle.det_log(np.ascontiguousarray(det, np.float32).ravel()).reshape(np.shape(det))
    hl = F(0.5) * lg
    t = F(0.5) * maha
    t = F(0.0) - t
    t = t - hl
    ll = t - F(1.8378770664)
    return o0, o1, o2, o3, o4, ll


def sum_loglik(terms):
    """terms [n][L] float32 (0 where a landmark adds nothing) -> [n]: landmark l goes to accumulator l mod 128 in order of l,
    accumulators j and j + 64 are added, then the 6-level xor butterfly over the 64 sums."""
    n, L = terms.shape
    nslots = (L + LANES - 1) // LANES * LANES
    pad = np.zeros((n, nslots), np.float32)
    pad[:, :L] = terms
    pad = pad.reshape(n, nslots // LANES, LANES)
    lane = np.zeros((n, LANES), np.float32)
    for g in range(pad.shape[1]):
        lane = lane + pad[:, g]
    t = lane[:, :64] + lane[:, 64:]
    j = np.arange(64)
    s = 1
    while s < 64:
        t = t + t[:, j ^ s]
        s <<= 1
    return np.ascontiguousarray(t[:, 0])


def update(map_in, x, y, th, anc, obs_id, obs_zx, obs_zy, meas_cov, L=None, in_place=False):
    """map_in: float32 [rows][5][plane_stride >= L], one row per particle.  Out of place: row i of the result starts as a copy of
    row anc[i] (anc None: i) and gets the update of the observed landmarks; in place (anc must be None): the same on row i.
    First sighting (P_xx < 0): mean = w, P = R_w, no likelihood term.  -> (map_out [n][5][plane_stride], loglik [n]); the columns
    at and beyond L are copied along and mean nothing."""
    assert valid_cov(meas_cov)
    assert not (in_place and anc is not None)
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    n = len(x)
    L = map_in.shape[2] if L is None else L
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    out = map_in[src].copy()
    ids = np.asarray(obs_id, np.int64)
    terms = np.zeros((n, L), np.float32)
    if len(ids) == 0:
        return out, sum_loglik(terms)
    assert len(np.unique(ids)) == len(ids) and ids.min() >= 0 and ids.max() < L
    s, c = oracle.det_sincos(th)
    rxx, rxy, ryy = world_noise(meas_cov, s, c)
    detq = det_q(meas_cov)
    col = lambda a: np.asarray(a, np.float32)[:, None]
    zx, zy = np.asarray(obs_zx, np.float32)[None, :], np.asarray(obs_zy, np.float32)[None, :]
    p = out[:, :, ids]                                              # [n][5][k] priors (a copy)
    first = p[:, 2] < 0
    with np.errstate(all="ignore"):                                 # (first sightings run through the arithmetic and are selected away)
        o0, o1, o2, o3, o4, ll = update_one(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], zx, zy, col(s), col(c), col(x), col(y),
                                            col(rxx), col(rxy), col(ryy), detq)
    wx, wy = observed_point(zx, zy, col(s), col(c), col(x), col(y))
    k = len(ids)
    full = lambda a: np.broadcast_to(col(a), (n, k))
    out[:, 0, ids] = np.where(first, wx, o0)
    out[:, 1, ids] = np.where(first, wy, o1)
    out[:, 2, ids] = np.where(first, full(rxx), o2)
    out[:, 3, ids] = np.where(first, full(rxy), o3)
    out[:, 4, ids] = np.where(first, full(ryy), o4)
    terms[:, ids] = np.where(first, F(0.0), ll)
    return out, sum_loglik(terms)


def frame_loop(world, n, frames, covs, *, seed, sigma, meas_var, score_gain, dp, observations, ess=0.0, refine=None):
    """The session's frame loop restated from the oracle's stage functions, with `update` above as its landmark stage: the
    executable statement of what a rows session does once slam_pf_meas_cov_set was called.  world: dict(meta, edt, bx, by, x, y,
    th, mp) (the first n particles are used); covs[f]: the (qxx, qxy, qyy) of frame f, or None for the isotropic update of
    orc_ekf_update with meas_var; observations(f) -> (ids, zx, zy); ess: the resample gate (0: every frame resamples);
    refine: (step_xy, step_theta, sweeps) or None.  -> one dict per frame: pose [3][n] and map [n][5][L] with the frame's
    resample applied (what slam_pf_get_poses_host / slam_pf_get_map_host return), logw, anc, resampled."""
    import _refine_spec as R

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    for f in range(frames):
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp, sigma, seed, f)
        if refine:
            x, y, th, score, _ = R.refine(oracle, world["meta"], world["edt"], world["bx"], world["by"], x, y, th, *refine)
        else:
            score, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        ids, zx, zy = observations(f)
        if covs[f] is None:
            mp, ll = oracle.ekf_update(mp, x, y, th, anc, ids, zx, zy, meas_var)
        else:
            mp, ll = update(mp, x, y, th, anc, ids, zx, zy, covs[f])
        logw, m = oracle.logweight_carry(score, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled))
    return out
