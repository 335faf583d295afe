"""The specification of data association under a 2x2 sensor-frame measurement covariance (include/slam_hip.h:
slam_associate_aniso_dev, slam_ekf_update_assoc_aniso_dev, slam_pf_assoc_cov_set) in numpy float32, one rounded operation per
line.  TEST INFRASTRUCTURE shared by test_assoc_aniso_spec_cpu.py, test_assoc_aniso_behaviour_cpu.py and the GPU tests.  It is
tests/_assoc_spec.py with S = P + R_w(theta_i) in the place of P + q I: the world-frame noise, det Q, the landmark update and the
log-likelihood's summation come from tests/_aniso_spec.py, the observed point, the cost of a pair and the table's conventions
from tests/_assoc_spec.py, and nothing from the package.

Particle i with (s, c) = det_sincos(theta_i) and R_w = (rxx, rxy, ryy) = world_noise(Q, s, c) gates, matches, creates and updates
with that R_w: the cost m(l, k) is the very Mahalanobis term of _aniso_spec.update_one's likelihood, and a landmark it creates
starts with P = R_w.
"""
import numpy as np

import oracle
import _aniso_spec as S
import _assoc_spec as A

F = np.float32
NONE = A.NONE
MAX_DETECTIONS = A.MAX_DETECTIONS


def shared(p, rxx, rxy, ryy):
    """p [n][5][L] priors, R_w [n][1] -> (seen, mx, my, i00, i01, i11), [n][L] each, the tuple _assoc_spec.cost takes: which
    landmarks take part (not P_xx < 0) and (P + R_w)^-1 with the operations of _aniso_spec.update_one, in its order."""
    mx, my, pxx, pxy, pyy = (p[:, j] for j in range(5))
    seen = ~(pxx < 0)
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
    return seen, mx, my, i00, i01, i11


def _prepare(map_in, x, y, th, anc, zx, zy, meas_cov, L):
    """Steps a and b up to the per-landmark part: -> (src rows [n][5][L], the tuple of shared(), wx, wy [n][K])."""
    s, c = oracle.det_sincos(th)
    rxx, rxy, ryy = S.world_noise(meas_cov, s, c)
    col = lambda a: np.asarray(a, np.float32)[:, None]
    wx, wy = A.observed_point(zx[None, :], zy[None, :], col(s), col(c), col(x), col(y))
    src = np.arange(len(x)) if anc is None else np.asarray(anc, np.int64)
    with np.errstate(all="ignore"):
        sh = shared(map_in[src][:, :, :L], col(rxx), col(rxy), col(ryy))
    return sh, wx, wy


def cost_matrix(map_in, x, y, th, anc, zx, zy, meas_cov, L=None):
    """-> (seen bool [n][L], m float32 [n][L][K]): the cost of every (landmark, detection) pair as associate() sees it (NaN and
    junk where a landmark is not seen)."""
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    L = map_in.shape[2] if L is None else L
    sh, wx, wy = _prepare(map_in, x, y, th, anc, zx, zy, meas_cov, L)
    with np.errstate(all="ignore"):
        m = np.stack([A.cost(sh, wx[:, k:k + 1], wy[:, k:k + 1]) for k in range(len(zx))], axis=2) if len(zx) else np.empty((len(x), L, 0), np.float32)
    return sh[0], m


def associate(map_in, x, y, th, anc, zx, zy, meas_cov, gate, new_gate, create, L=None, assoc_stride=None):
    """_assoc_spec.associate with meas_cov = (qxx, qxy, qyy) in the place of meas_var; steps c to f word for word.
    -> (assoc uint8 [n][assoc_stride], stats int32 [n][3] = matched, created, dropped)."""
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n, K = len(x), len(zx)
    L = map_in.shape[2] if L is None else L
    stride = L if assoc_stride is None else assoc_stride
    gate, new_gate = F(gate), F(new_gate)
    assert K <= MAX_DETECTIONS and stride >= L and np.isfinite(gate) and gate > 0 and new_gate >= gate and S.valid_cov(meas_cov)
    assoc = np.full((n, stride), NONE, np.uint8)
    stats = np.zeros((n, 3), np.int32)
    if K == 0:
        return assoc, stats
    # a. world-frame points, once per (particle, detection); b. what the seen landmarks share over the detections
    sh, wx, wy = _prepare(map_in, x, y, th, anc, zx, zy, meas_cov, L)
    seen = sh[0]
    # c. the landmark chooses: its cheapest detection, the lowest k on ties (a strict "<" walking k upwards from +inf: NaN never wins)
    best = np.full((n, L), np.inf, np.float32)
    bk = np.zeros((n, L), np.int64)
    near = np.zeros((n, K), bool)   # (for e: some seen landmark lies within new_gate of detection k)
    with np.errstate(all="ignore"):
        for k in range(K):
            m = A.cost(sh, wx[:, k:k + 1], wy[:, k:k + 1])
            take = m < best
            best = np.where(take, m, best)
            bk = np.where(take, k, bk)
            near[:, k] = (seen & (m <= new_gate)).any(axis=1)
    cand = seen & (best >= 0) & (best <= gate)
    # d. the detection chooses: among the candidates that chose it the cheapest, the lowest l on ties (argmin: the first minimum)
    matched = np.zeros((n, K), bool)
    rows_i = np.arange(n)
    for k in range(K):
        mine = cand & (bk == k)
        has = mine.any(axis=1)
        if L == 0 or not has.any():
            continue
        l = np.argmin(np.where(mine, best, np.inf), axis=1)
        assoc[rows_i[has], l[has]] = k
        matched[:, k] = has
    stats[:, 0] = matched.sum(axis=1)
    # e. new landmarks: unmatched detections with no seen landmark within new_gate take the unseen slots, both in ascending order
    if create:
        new = ~matched & ~near
        for i in np.flatnonzero(new.any(axis=1)):
            slots = np.flatnonzero(~seen[i])
            ks = np.flatnonzero(new[i])
            cnt = min(len(slots), len(ks))
            assoc[i, slots[:cnt]] = ks[:cnt]
            stats[i, 1] = cnt
    stats[:, 2] = K - stats[:, 0] - stats[:, 1]
    return assoc, stats


def update(map_in, x, y, th, anc, assoc, zx, zy, meas_cov, L=None, in_place=False):
    """The landmark update under a per-particle table and R_w: particle i gets _aniso_spec.update with its own observation list
    {(l, z[assoc[i][l]]) : assoc[i][l] names a detection} (test_assoc_aniso_spec_cpu.py holds it to exactly that, particle by
    particle).  Written on whole arrays with _aniso_spec's own functions: every element sees the operations of that call, so the bits
    are its bits.  Out of place row i starts as a copy of row anc[i] (anc None: i); in place (anc must be None) the same on row i.
    A first sighting (P_xx < 0) stores w and P = R_w(theta_i), no likelihood term.  -> (map_out [n][5][plane_stride], loglik [n])."""
    assert S.valid_cov(meas_cov)
    assert not (in_place and anc is not None)
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n, K = len(x), len(zx)
    L = map_in.shape[2] if L is None else L
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    out = map_in[src].copy()
    terms = np.zeros((n, L), np.float32)
    a = np.asarray(assoc)[:n, :L].astype(np.int64)
    has = a < K                                                      # (an entry that names no detection counts as NONE)
    if K == 0 or not has.any():
        return out, S.sum_loglik(terms)
    k = np.where(has, a, 0)
    tzx, tzy = zx[k], zy[k]                                          # [n][L]: the particle's own observation of every landmark
    s, c = oracle.det_sincos(th)
    rxx, rxy, ryy = S.world_noise(meas_cov, s, c)
    detq = S.det_q(meas_cov)
    col = lambda v: np.asarray(v, np.float32)[:, None]
    p = out[:, :, :L].copy()
    first = p[:, 2] < 0
    with np.errstate(all="ignore"):                                  # (everything runs through the arithmetic and is selected away)
        o0, o1, o2, o3, o4, ll = S.update_one(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], tzx, tzy, col(s), col(c), col(x), col(y),
                                              col(rxx), col(rxy), col(ryy), detq)
        wx, wy = S.observed_point(tzx, tzy, col(s), col(c), col(x), col(y))
    full = lambda v: np.broadcast_to(col(v), (n, L))
    for j, (f, o) in enumerate(((wx, o0), (wy, o1), (full(rxx), o2), (full(rxy), o3), (full(ryy), o4))):
        out[:, j, :L] = np.where(has, np.where(first, f, o), p[:, j])
    terms = np.where(has & ~first, ll, F(0.0)).astype(np.float32)
    return out, S.sum_loglik(terms)


def frame_loop(world, n, frames, *, seed, sigma, meas_cov, score_gain, dp, detections, gate, new_gate, create, prune=None, ess=0.0,
               refine=None, score=True, ev0=None):
    """_assoc_spec.frame_loop with the two stages above in place of its own — what a rows session does once
    slam_pf_assoc_cov_set was called — and, with prune = (hit, miss, cmax, view_range) (or a function of the frame number that
    returns that or None), _evidence_spec.evidence behind the update exactly as _evidence_spec.frame_loop applies it behind the
    isotropic one (slam_pf_prune_set).  detections(f) -> (zx, zy), or None: a frame without a detection hand-over.
    -> one dict per frame as _assoc_spec.frame_loop's, plus ev / ev_raw / ev_stats as _evidence_spec.frame_loop's (None without)."""
    import _evidence_spec as E
    import _refine_spec as R

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    ev, was_on = ev0, False
    for f in range(frames):
        pr = prune(f) if callable(prune) else prune
        if pr and not was_on and (ev is None or f > 0):
            ev = E.evidence_init(mp, pr[2])
        was_on = bool(pr)
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], world["bx"], world["by"], x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        det = detections(f)
        assoc = stats = ev_stats = None
        if det is None:
            if anc is not None:
                mp = mp[anc]
                ev = ev[anc] if pr else ev
            ll = None
        else:
            zx, zy = det
            assoc, stats = associate(mp, x, y, th, anc, zx, zy, meas_cov, gate, new_gate, create)
            mp, ll = update(mp, x, y, th, anc, assoc, zx, zy, meas_cov)
            if pr:
                mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, len(zx), ev, *pr)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if pr else None, ev_raw=ev if pr else None, ev_stats=ev_stats))
    return out
