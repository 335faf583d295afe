"""The specification of data association under a measurement covariance PER DETECTION (include/slam_hip.h:
slam_detections_cov_upload_host, slam_associate_detcov_dev, slam_ekf_update_assoc_detcov_dev) in numpy float32, one rounded
operation per line.  TEST INFRASTRUCTURE shared by test_assoc_detcov_spec_cpu.py and the GPU tests.  It is
tests/_assoc_aniso_spec.py with Q_k = (qxx[k], qxy[k], qyy[k]) of detection k in the place of the one Q, and nothing else changes:
the world-frame noise, det Q, the landmark update and the log-likelihood's summation come from tests/_aniso_spec.py, (P + R_w)^-1
from tests/_assoc_aniso_spec.py, the observed point, the cost of a pair and the table's conventions from tests/_assoc_spec.py, and
nothing from the package.

Particle i with (s, c) = det_sincos(theta_i) forms R_w(i, k) = world_noise(Q_k, s, c).  The cost m(l, k) of a (landmark,
detection) pair is the very Mahalanobis term of _aniso_spec.update_one's likelihood under R_w(i, k) — (P + R_w(i, k))^-1 is formed
per pair, through the same reciprocal — the update of landmark l runs with R_w(i, assoc[i][l]) and det Q of that detection, and a
landmark a detection creates starts with P = R_w(i, k) of that detection.
"""
import numpy as np

import oracle
import _aniso_spec as S
import _assoc_aniso_spec as AA
import _assoc_spec as A

F = np.float32
NONE = A.NONE
MAX_DETECTIONS = A.MAX_DETECTIONS


def covs_of(meas_covs, K):
    """meas_covs: (qxx, qxy, qyy), three sequences of K values -> three float32 arrays [K]."""
    qxx, qxy, qyy = (np.ascontiguousarray(v, np.float32) for v in meas_covs)
    assert qxx.shape == qxy.shape == qyy.shape == (K,)
    return qxx, qxy, qyy


def valid_covs(meas_covs):
    """Every Q_k by the rule of _aniso_spec.valid_cov."""
    qxx, qxy, qyy = (np.asarray(v, np.float32) for v in meas_covs)
    return all(S.valid_cov((qxx[k], qxy[k], qyy[k])) for k in range(len(qxx)))


def _pose(x, y, th, zx, zy):
    """Step a: (s, c) [n] and the world-frame points wx, wy [n][K]."""
    s, c = oracle.det_sincos(th)
    col = lambda a: np.asarray(a, np.float32)[:, None]
    wx, wy = A.observed_point(zx[None, :], zy[None, :], col(s), col(c), col(x), col(y))
    return s, c, wx, wy


def shared_k(p, s, c, q_k):
    """Step b of one detection: p [n][5][L] priors, (s, c) [n], Q_k -> the tuple _assoc_spec.cost takes, with (P + R_w(i, k))^-1."""
    col = lambda a: np.asarray(a, np.float32)[:, None]
    rxx, rxy, ryy = S.world_noise(q_k, s, c)
    return AA.shared(p, col(rxx), col(rxy), col(ryy))


def cost_matrix(map_in, x, y, th, anc, zx, zy, meas_covs, L=None):
    """-> (seen bool [n][L], m float32 [n][L][K]): the cost of every (landmark, detection) pair as associate() sees it."""
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    K = len(zx)
    qxx, qxy, qyy = covs_of(meas_covs, K)
    L = map_in.shape[2] if L is None else L
    s, c, wx, wy = _pose(x, y, th, zx, zy)
    src = np.arange(len(x)) if anc is None else np.asarray(anc, np.int64)
    p = map_in[src][:, :, :L]
    m = np.empty((len(x), L, K), np.float32)
    with np.errstate(all="ignore"):
        for k in range(K):
            m[:, :, k] = A.cost(shared_k(p, s, c, (qxx[k], qxy[k], qyy[k])), wx[:, k:k + 1], wy[:, k:k + 1])
    return ~(p[:, 2] < 0), m


def associate(map_in, x, y, th, anc, zx, zy, meas_covs, gate, new_gate, create, L=None, assoc_stride=None):
    """_assoc_aniso_spec.associate with Q_k per detection; steps a and c to f word for word.
    -> (assoc uint8 [n][assoc_stride], stats int32 [n][3] = matched, created, dropped)."""
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n, K = len(x), len(zx)
    qxx, qxy, qyy = covs_of(meas_covs, K)
    L = map_in.shape[2] if L is None else L
    stride = L if assoc_stride is None else assoc_stride
    gate, new_gate = F(gate), F(new_gate)
    assert K <= MAX_DETECTIONS and stride >= L and np.isfinite(gate) and gate > 0 and new_gate >= gate and valid_covs((qxx, qxy, qyy))
    assoc = np.full((n, stride), NONE, np.uint8)
    stats = np.zeros((n, 3), np.int32)
    if K == 0:
        return assoc, stats
    # a. world-frame points, once per (particle, detection)
    s, c, wx, wy = _pose(x, y, th, zx, zy)
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    p = map_in[src][:, :, :L]
    seen = ~(p[:, 2] < 0)
    # c. the landmark chooses: its cheapest detection, the lowest k on ties (a strict "<" walking k upwards from +inf: NaN never wins)
    best = np.full((n, L), np.inf, np.float32)
    bk = np.zeros((n, L), np.int64)
    near = np.zeros((n, K), bool)   # (for e: some seen landmark lies within new_gate of detection k)
    with np.errstate(all="ignore"):
        for k in range(K):
            # b. (P + R_w(i, k))^-1 per (landmark, detection) pair
            sh = shared_k(p, s, c, (qxx[k], qxy[k], qyy[k]))
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


def update(map_in, x, y, th, anc, assoc, zx, zy, meas_covs, L=None, in_place=False):
    """_assoc_aniso_spec.update with, for landmark l of particle i, R_w(i, assoc[i][l]) and det Q of that detection: particle i
    gets _aniso_spec.update once per distinct detection k its table names, with Q_k (test_assoc_detcov_spec_cpu.py holds it to
    exactly that).  A first sighting stores w and P = R_w(i, k), no likelihood term.
    -> (map_out [n][5][plane_stride], loglik [n])."""
    assert not (in_place and anc is not None)
    map_in = np.ascontiguousarray(map_in, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, np.float32), np.ascontiguousarray(zy, np.float32)
    n, K = len(x), len(zx)
    qxx, qxy, qyy = covs_of(meas_covs, K)
    assert valid_covs((qxx, qxy, qyy))
    L = map_in.shape[2] if L is None else L
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    out = map_in[src].copy()
    terms = np.zeros((n, L), np.float32)
    a = np.asarray(assoc)[:n, :L].astype(np.int64)
    has = a < K                                                      # (an entry that names no detection counts as NONE)
    if K == 0 or not has.any():
        return out, S.sum_loglik(terms)
    k = np.where(has, a, 0)
    tzx, tzy = zx[k], zy[k]                                          # [n][L]: the particle's own observation of every landmark ...
    tq = (qxx[k], qxy[k], qyy[k])                                    # ... and that detection's covariance
    s, c = oracle.det_sincos(th)
    col = lambda v: np.asarray(v, np.float32)[:, None]
    rxx, rxy, ryy = S.world_noise(tq, col(s), col(c))                # [n][L]
    detq = S.det_q(tq)
    p = out[:, :, :L].copy()
    first = p[:, 2] < 0
    with np.errstate(all="ignore"):                                  # (everything runs through the arithmetic and is selected away)
        o0, o1, o2, o3, o4, ll = S.update_one(p[:, 0], p[:, 1], p[:, 2], p[:, 3], p[:, 4], tzx, tzy, col(s), col(c), col(x), col(y),
                                              rxx, rxy, ryy, detq)
        wx, wy = S.observed_point(tzx, tzy, col(s), col(c), col(x), col(y))
    for j, (f, o) in enumerate(((wx, o0), (wy, o1), (rxx, o2), (rxy, o3), (ryy, o4))):
        out[:, j, :L] = np.where(has, np.where(first, f, o), p[:, j])
    terms = np.where(has & ~first, ll, F(0.0)).astype(np.float32)
    return out, S.sum_loglik(terms)


def frame_loop(world, n, frames, *, seed, sigma, score_gain, dp, detections, gate, new_gate, create, prune=None, ess=0.0, refine=None,
               score=True, ev0=None):
    """_assoc_aniso_spec.frame_loop with the two stages above in place of its own — what a rows session does once
    slam_pf_assoc_detcov_set was called.  detections(f) -> (zx, zy, (qxx, qxy, qyy)), or None: a frame without a detection
    hand-over.  Everything else, pruning included, as there.  -> one dict per frame as _assoc_aniso_spec.frame_loop's."""
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
            zx, zy, covs = det
            assoc, stats = associate(mp, x, y, th, anc, zx, zy, covs, gate, new_gate, create)
            mp, ll = update(mp, x, y, th, anc, assoc, zx, zy, covs)
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
