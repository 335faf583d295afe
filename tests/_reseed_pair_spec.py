"""The specification of reseeding from detection PAIRS ("Reseeding from detection pairs"; include/slam_hip.h:
slam_pose_reseed_pairs_dev, slam_pf_known_map_reseed_pairs) in numpy float32.  TEST INFRASTRUCTURE shared by
test_reseed_pair_spec_cpu.py, test_reseed_pair_behaviour_cpu.py and the GPU tests.

_reseed_spec.reseed pins the robot to a circle: ONE detection on ONE landmark, the heading drawn blind.  Two detections k1, k2 on
two landmarks j1, j2 fix the pose completely, and the pairing can be checked before the proposal is made: |z_k2 - z_k1| must be
|m_j2 - m_j1|.  j1, k1, k2 are drawn; j2 is SEARCHED for among the landmarks whose distance from m_j1 is the detections' distance
within tol, and one of them is drawn; the heading is the angle of a = z_k2 - z_k1 less the angle of b = m_j2 - m_j1 (the update's
convention, _assoc_spec.observed_point: the world offset of a detection is (c zx + s zy, c zy - s zx), the sensor vector turned by
MINUS theta), and the position is _reseed_spec.propose of (m_j1, z_k1).  Every product, sum, difference, quotient and square root
is one float32 rounding, in the order written here.

Composes _reseed_spec (philox, threshold, propose, the flag constants) and oracle.det_sincos; det_atan2 is new and defined here.
Philox stream 2 is the reseed stream (the SAME slots are chosen as _reseed_spec.reseed chooses); stream 3 picks the partner.
"""
import numpy as np

import _reseed_spec as R

F = np.float32
STREAM_PARTNER = 3
REPLACED, CHOSEN_EMPTY, TOO_CLOSE, NO_PARTNER = R.REPLACED, R.CHOSEN_EMPTY, 3, 4
TAN_PI_8 = F(0.4142135623730950)
PI_4, PI_2, PI = F(0.7853981634), F(1.5707963268), F(3.1415926536)
ATAN_COEF = (F(8.05374449538e-2), F(1.38776856032e-1), F(1.99777106478e-1), F(3.33329491539e-1))


def det_atan2(y, x):
    """The specified atan2 on float32 arrays -> float32 in [-pi, pi] (as rounded).  (0, 0) is outside its domain and asserted.
        hi = max(|x|, |y|), lo = the other (|y| > |x|: swapped);  t = lo / hi            one correctly rounded division, t in [0, 1]
        t > tan(pi/8):  y0 = pi/4,  t = (t - 1) / (t + 1);  else y0 = 0                  the Cephes atanf reduction that can arise
        z = t t;  p = ((((c0 z - c1) z + c2) z - c3) z) t + t;  r = y0 + p               Cephes' four coefficients, Horner
        swapped: r = pi/2 - r;   x < 0: r = pi - r;   y < 0: r = -r                      the octants
    every operation rounded on its own."""
    y, x = np.broadcast_arrays(np.asarray(y, F), np.asarray(x, F))
    ax, ay = np.abs(x), np.abs(y)
    swap = ay > ax
    hi = np.where(swap, ay, ax)
    lo = np.where(swap, ax, ay)
    assert np.all(hi > 0), "det_atan2(0, 0)"
    t = lo / hi
    red = t > TAN_PI_8
    num = t - F(1.0)
    den = t + F(1.0)
    t = np.where(red, num / den, t).astype(F)
    y0 = np.where(red, PI_4, F(0.0)).astype(F)
    z = t * t
    p = ATAN_COEF[0] * z
    p = p - ATAN_COEF[1]
    p = p * z
    p = p + ATAN_COEF[2]
    p = p * z
    p = p - ATAN_COEF[3]
    p = p * z
    p = p * t
    p = p + t
    r = y0 + p
    r = np.where(swap, PI_2 - r, r).astype(F)
    r = np.where(x < 0, PI - r, r).astype(F)
    r = np.where(y < 0, -r, r).astype(F)
    return r


def draws(n, first_id, seed, frame, L, K):
    """-> (r0 uint32 [n], j1, k1, k2 int64 [n], rb0 uint32 [n]) of the slots first_id .. first_id + n - 1; K >= 2."""
    gid = (np.arange(n, dtype=np.uint64) + np.uint64(first_id))
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    lo, hi = gid & np.uint64(0xffffffff), gid >> np.uint64(32)
    ra = R.philox(lo, hi, frame, R.STREAM, *key)
    rb = R.philox(lo, hi, frame, STREAM_PARTNER, *key)
    sh = np.uint64(32)
    j1 = ((ra[1].astype(np.uint64) * np.uint64(L)) >> sh).astype(np.int64)        # umulhi(rA1, L)
    k1 = ((ra[2].astype(np.uint64) * np.uint64(K)) >> sh).astype(np.int64)        # umulhi(rA2, K)
    k2 = ((ra[3].astype(np.uint64) * np.uint64(K - 1)) >> sh).astype(np.int64)    # umulhi(rA3, K - 1): one of the others
    k2 = k2 + (k2 >= k1)
    return ra[0], j1, k1, k2, rb[0]


def partners(M, j1, lo2, hi2):
    """-> bool [L]: the landmarks that can stand where the second detection is, for ONE slot.  Squared distances only."""
    bx = M[0] - M[0][j1]
    by = M[1] - M[1][j1]
    t = bx * bx
    u = by * by
    dm2 = t + u
    ok = ~(M[2] < 0) & (dm2 > 0) & (lo2 <= dm2) & (dm2 <= hi2)
    ok[j1] = False
    return ok


def reseed_pairs(M, x, y, th, anc, zx, zy, first_id, seed, frame, fraction, tol, min_sep):
    """-> (x', y', th', flag uint8 [n], counts int32 [4] = replaced, j1 empty, too close, no partner).  anc int32 [n] or None
    (identity).  flag: 1 replaced, 2 chosen but landmark slot j1 is empty, 3 chosen but the two detections are closer than min_sep
    (or not numbers), 4 chosen but no landmark stands at the detections' distance from j1, 0 not chosen.  K < 2: None (nothing is
    written), counts 0."""
    import oracle

    M = np.ascontiguousarray(M, F)
    x, y, th = (np.ascontiguousarray(a, F) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, F), np.ascontiguousarray(zy, F)
    n, L, K = len(x), M.shape[1], len(zx)
    tol, min_sep = F(tol), F(min_sep)
    if not (M.shape[0] == 5 and L >= 2 and K <= 64 and len(zy) == K and n >= 1 and tol >= 0 and min_sep > tol and np.isfinite(min_sep)):
        raise ValueError("shapes or parameters")
    thr = R.threshold(fraction)
    if K < 2:
        return None, None, None, None, np.zeros(4, np.int32)
    min_sep2 = min_sep * min_sep
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    r0, j1, k1, k2, rb0 = draws(n, first_id, seed, frame, L, K)
    chosen = r0.astype(np.uint64) < np.uint64(thr)
    with np.errstate(invalid="ignore", over="ignore"):
        ax = zx[k2] - zx[k1]
        ay = zy[k2] - zy[k1]
        t = ax * ax
        u = ay * ay
        dz2 = t + u
        close = chosen & ~(dz2 >= min_sep2)          # (a NaN is too close)
        empty = chosen & ~close & (M[2][j1] < 0)
        search = chosen & ~close & ~empty
        dz = np.sqrt(dz2)
        lo = dz - tol
        hi = dz + tol
        lo2 = lo * lo
        hi2 = hi * hi
    flag = np.where(close, TOO_CLOSE, np.where(empty, CHOSEN_EMPTY, 0)).astype(np.uint8)
    xo, yo, to = x[src].copy(), y[src].copy(), th[src].copy()
    j2 = np.full(n, -1, np.int64)
    for i in np.flatnonzero(search):
        ok = np.flatnonzero(partners(M, j1[i], lo2[i], hi2[i]))   # ascending j
        if len(ok) == 0:
            flag[i] = NO_PARTNER
            continue
        c = (int(rb0[i]) * len(ok)) >> 32                         # umulhi(rB0, cnt)
        j2[i] = ok[c]
        flag[i] = REPLACED
    rep = np.flatnonzero(flag == REPLACED)
    if len(rep):
        a, b = j1[rep], j2[rep]
        bx = M[0][b] - M[0][a]
        by = M[1][b] - M[1][a]
        vx, vy = ax[rep], ay[rep]
        t = bx * vy
        u = by * vx
        cr = t - u
        t = vx * bx
        u = vy * by
        dt = t + u
        theta = det_atan2(cr, dt)
        theta = np.where(theta < 0, theta + R.TWO_PI, theta).astype(F)
        s, c = oracle.det_sincos(theta)
        xo[rep], yo[rep] = R.propose(M[0][a], M[1][a], zx[k1[rep]], zy[k1[rep]], s, c)
        to[rep] = theta
    counts = np.array([int((flag == v).sum()) for v in (REPLACED, CHOSEN_EMPTY, TOO_CLOSE, NO_PARTNER)], np.int32)
    return xo, yo, to, flag, counts


def frame_loop(world, n, frames, *, seed, sigma, score_gain, dp, detections, known_map, gate, log_clutter, tol, min_sep,
               reseed_after=None, meas_var=None, ess=0.0, score=True, scans=None):
    """_reseed_spec.frame_loop with reseed_pairs in place of reseed between frames — what a session does whose host calls
    slam_pf_known_map_reseed_pairs behind the frames reseed_after(f) names.  A frame with fewer than two detections is not reseeded
    (the call writes nothing): its counts are 0 and reseeded is None.  counts int32 [4]."""
    import oracle
    import _localise_detcov_spec as SD
    import _localise_spec as S

    x, y, th = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    for f in range(frames):
        bx, by = scans[f] if scans is not None else (world.get("bx"), world.get("by"))
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        sc = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)[0] if score else np.zeros(n, np.float32)
        M = known_map(f) if callable(known_map) else known_map
        det = detections(f)
        assoc = stats = ll = None
        if M is not None and det is not None:
            if meas_var is None:
                assoc, stats, ll = SD.localise(M, x, y, th, det[0], det[1], det[2], gate, log_clutter)
            else:
                assoc, stats, ll = S.localise(M, x, y, th, det[0], det[1], meas_var, gate, log_clutter)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        fr = dict(pose=np.stack([x[anc], y[anc], th[anc]]), logw=logw, anc=anc, resampled=prev_resampled, assoc=assoc, stats=stats, ll=ll,
                  counts=None, reseeded=None)
        fraction = reseed_after(f) if reseed_after else None
        if fraction is not None and M is not None and det is not None:
            if len(det[0]) < 2:
                fr["counts"] = np.zeros(4, np.int32)
            else:
                x, y, th, _, fr["counts"] = reseed_pairs(M, x, y, th, anc, det[0], det[1], 0, seed, f + 1, fraction, tol, min_sep)
                anc, prev_resampled = None, True   # nothing is pending, no weight is carried
                fr["reseeded"] = np.stack([x, y, th])
        out.append(fr)
    return out
