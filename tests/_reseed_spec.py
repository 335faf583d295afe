"""The specification of reseeding the particle cloud from what the lidar sees ("Reseeding in a known map";
include/slam_hip.h: slam_pose_reseed_dev, slam_pf_known_map_reseed) in numpy float32.  TEST INFRASTRUCTURE shared by
test_reseed_spec_cpu.py, test_reseed_behaviour_cpu.py and the GPU tests.

A chosen fraction of the slots is replaced by pose proposals at each of which ONE detection of the frame coincides with ONE landmark
of the known map: landmark j, detection k and the heading theta are drawn, the position follows from the update's own convention
w = p + H^T z (_assoc_spec.observed_point) read backwards, p = m_j - H(theta)^T z_k.  Every product and sum is one float32 rounding.

The known map is M float32 [5][L]: planes mx, my, P_xx, P_xy, P_yy as in a row; a slot with P_xx < 0 holds no landmark.
Philox stream 2 is the reseed stream (0: motion, 1: resample, oracle/slam_oracle_pf.c).
"""
import numpy as np

F = np.float32
STREAM = 2
TWO_PI = F(6.2831853072)
REPLACED, CHOSEN_EMPTY = 1, 2


def philox(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on arrays of counters (uint32 each; scalars broadcast) -> four uint32 arrays.  oracle.philox, vectorised:
    `reseed` checks its first and last slot against that one on every call, test_reseed_spec_cpu.py many more."""
    c0, c1, c2, c3 = (np.asarray(c, np.uint64) & np.uint64(0xffffffff) for c in np.broadcast_arrays(c0, c1, c2, c3))
    k0, k1 = int(k0) & 0xffffffff, int(k1) & 0xffffffff
    lo32, sh = np.uint64(0xffffffff), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> sh) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> sh) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & lo32, n2, p0 & lo32
        k0 = (k0 + 0x9E3779B9) & 0xffffffff
        k1 = (k1 + 0xBB67AE85) & 0xffffffff
    return tuple(c.astype(np.uint32) for c in (c0, c1, c2, c3))


def threshold(fraction):
    """thr = floor(fraction * 2^32), in double, held in 64 bits: fraction in (0, 1]; 1 gives 2^32 — every slot is chosen."""
    fraction = float(fraction)
    if not (0.0 < fraction <= 1.0):   # (false for NaN)
        raise ValueError("fraction must lie in (0, 1]")
    return int(np.floor(np.float64(fraction) * np.float64(4294967296.0)))


def draws(n, first_id, seed, frame, L, K):
    """-> (r0 uint32 [n], j int64 [n], k int64 [n], theta float32 [n]) of the slots first_id .. first_id + n - 1."""
    import oracle

    gid = (np.arange(n, dtype=np.uint64) + np.uint64(first_id))
    key = (seed & 0xffffffff, (seed >> 32) & 0xffffffff)
    r = philox(gid & np.uint64(0xffffffff), gid >> np.uint64(32), frame, STREAM, *key)
    for i in {0, n - 1}:   # the vectorised generator against the oracle's
        g = int(first_id) + i
        want = oracle.philox([g & 0xffffffff, (g >> 32) & 0xffffffff, frame, STREAM], key)
        assert all(int(r[q][i]) == int(want[q]) for q in range(4)), "philox"
    j = (r[1].astype(np.uint64) * np.uint64(L)) >> np.uint64(32)     # umulhi(r1, L)
    k = (r[2].astype(np.uint64) * np.uint64(K)) >> np.uint64(32)     # umulhi(r2, K)
    u = (r[3] >> np.uint32(8)).astype(F) * F(5.9604644775390625e-8)  # 24 bits: exact
    return r[0], j.astype(np.int64), k.astype(np.int64), TWO_PI * u


def propose(mx, my, zx, zy, s, c):
    """The pose at which the detection (zx, zy) is seen exactly at (mx, my) under the heading whose sine and cosine are s, c:
    observed_point read backwards, one float32 rounding per operation, in this order."""
    mx, my, zx, zy, s, c = (np.asarray(a, F) for a in (mx, my, zx, zy, s, c))
    t = c * zx
    v = s * zy
    t = t + v
    x = mx - t
    t = c * zy
    v = s * zx
    t = t - v
    y = my - t
    return x, y


def reseed(M, x, y, th, anc, zx, zy, first_id, seed, frame, fraction):
    """-> (x', y', th', flag uint8 [n], counts int32 [2] = replaced, chosen but not replaced).  anc int32 [n] or None (identity):
    the pending resample, applied to the slots that are not replaced.  flag: 1 replaced, 2 chosen but its landmark slot is empty,
    0 otherwise.  No jitter is added: the next frame's motion sample spreads the proposals."""
    import oracle

    M = np.ascontiguousarray(M, F)
    x, y, th = (np.ascontiguousarray(a, F) for a in (x, y, th))
    zx, zy = np.ascontiguousarray(zx, F), np.ascontiguousarray(zy, F)
    n, L, K = len(x), M.shape[1], len(zx)
    if not (M.shape[0] == 5 and L >= 1 and 1 <= K <= 64 and len(zy) == K and n >= 1):
        raise ValueError("shapes")
    thr = threshold(fraction)
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    r0, j, k, theta = draws(n, first_id, seed, frame, L, K)
    chosen = r0.astype(np.uint64) < np.uint64(thr)
    s, c = oracle.det_sincos(theta)
    px, py = propose(M[0][j], M[1][j], zx[k], zy[k], s, c)
    replaced = chosen & ~(M[2][j] < 0)
    flag = np.where(replaced, REPLACED, np.where(chosen, CHOSEN_EMPTY, 0)).astype(np.uint8)
    xo = np.where(replaced, px, x[src]).astype(F)
    yo = np.where(replaced, py, y[src]).astype(F)
    to = np.where(replaced, theta, th[src]).astype(F)
    counts = np.array([int(replaced.sum()), int((chosen & ~replaced).sum())], np.int32)
    return xo, yo, to, flag, counts


def frame_loop(world, n, frames, *, seed, sigma, score_gain, dp, detections, known_map, gate, log_clutter, reseed_after=None,
               meas_var=None, ess=0.0, score=True, scans=None):
    """_localise_spec.frame_loop (meas_var given) or _localise_detcov_spec.frame_loop (meas_var None: detections(f) carries the
    covariances as its third entry), step for step, extended by `reseed` BETWEEN frames — what a session does whose host calls
    slam_pf_known_map_reseed behind the frames reseed_after(f) names: reseed_after(f) -> fraction or None.  The reseed reads the
    frame's poses through its resample, with the detections of that frame, under the frame word of the NEXT frame (the session's
    counter after the step); it leaves no pending resample and drops the weights a kept frame would carry.
    -> one dict per frame as there (pose: the frame's poses with its resample applied, as the host reads them before it reseeds),
    plus counts and reseeded [3][n], the population the reseed left (both None where no reseed ran)."""
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
        if fraction is not None and M is not None and det is not None and len(det[0]) > 0:
            x, y, th, _, fr["counts"] = reseed(M, x, y, th, anc, det[0], det[1], 0, seed, f + 1, fraction)
            anc, prev_resampled = None, True   # nothing is pending, no weight is carried
            fr["reseeded"] = np.stack([x, y, th])
        out.append(fr)
    return out
