"""The specification of line-of-sight evidence ("Line of sight"; include/slam_hip.h: slam_sight_table_dev,
slam_landmark_evidence_sight_dev, slam_pf_prune_sight_set) in float32 numpy, one rounded operation per line, no fused
multiply-add.  TEST INFRASTRUCTURE shared by test_sight_spec_cpu.py, test_sight_behaviour_cpu.py and the GPU tests.  It reuses
tests/_evidence_spec.py and tests/_detect_spec.py and nothing of the package.

The existence evidence of tests/_evidence_spec.py calls a landmark visible when it lies within view_range.  Here a landmark that
lies BEHIND what the frame's scan hit in its direction is HIDDEN: it takes no miss (a hit still counts).  Directions are `bins`
equal steps of the diamond angle p in [0, 4) of a sensor-frame point — monotone in the true angle, one division, no arctangent —
and the SIGHT TABLE of a scan holds, per bin, the smallest squared range of the scan's points in it.
"""
import numpy as np

import _evidence_spec as E

F = np.float32
MAX_BINS = 1024
BINS = (32, 64, 128, 256, 512, 1024)


def bin_of(x, y, bins):
    """-> (j int64, has bool): the bin of the sensor-frame points (x, y); has = False: the point has no bin (j = 0 there)."""
    assert bins in BINS
    x, y = np.asarray(x, F), np.asarray(y, F)
    with np.errstate(all="ignore"):
        ax = np.abs(x)
        ay = np.abs(y)
        s = ax + ay
        has = (s > 0) & np.isfinite(s)
        q = ay / np.where(has, s, F(1.0))
        q = np.where(has, q, F(0.0))
        neg_x, neg_y = x < 0, y < 0          # -0.0 is not negative
        p = np.where(neg_x, np.where(neg_y, F(2.0) + q, F(2.0) - q), np.where(neg_y, F(4.0) - q, q)).astype(F)
        k = p * F(bins // 4)                 # a power of two: exact
    j = k.astype(np.int64) & (bins - 1)      # p == 4 wraps to bin 0
    return np.where(has, j, 0), has


def table(bx, by, bins):
    """The sight table of a scan -> float32 [bins]: the minimum of r2 = x*x + y*y over the points of bin j, +inf: none."""
    x, y = np.ascontiguousarray(bx, F), np.ascontiguousarray(by, F)
    j, has = bin_of(x, y, bins)
    with np.errstate(all="ignore"):
        xx = x * x
        yy = y * y
        r2 = xx + yy
    T = np.full(bins, np.inf, F)
    np.minimum.at(T, j[has], r2[has])
    return T


def hidden(T, margin, px, py, th, mx, my):
    """px, py, th [n] (or [n][1]); mx, my [n][L] -> (hidden bool [n][L], bin [n][L], has [n][L])."""
    import oracle

    bins = len(T)
    T = np.ascontiguousarray(T, F)
    px, py, th = (np.ascontiguousarray(a, F).reshape(-1, 1) for a in (px, py, th))
    mx, my = np.asarray(mx, F), np.asarray(my, F)
    s, c = oracle.det_sincos(th.ravel())
    s, c = s.reshape(-1, 1), c.reshape(-1, 1)
    with np.errstate(all="ignore"):
        dx = mx - px
        dy = my - py
        t = dx * dx
        u = dy * dy
        r2 = t + u
        a = c * dx
        b = s * dy
        zx = a - b
        a = s * dx
        b = c * dy
        zy = a + b
        j, has = bin_of(zx, zy, bins)
        near = np.minimum(np.minimum(T[(j - 1) & (bins - 1)], T[j]), T[(j + 1) & (bins - 1)])
        r = np.sqrt(r2)
        g = r - F(margin)
        g2 = g * g
        hid = has & (g > 0) & (near < g2)
    return hid, j, has


def evidence(map_rows, x, y, th, anc, assoc, K, ev_in, hit, miss, cmax, view_range, T, margin, L=None, in_place=False):
    """_evidence_spec.evidence with miss_now = seen & ~hit_now & visible & ~hidden (T: the sight table, margin > 0).
    -> (map_out, ev_out, stats int32 [n][2], spared int32 [n] = landmarks with seen & ~hit_now & visible & hidden)."""
    assert not (in_place and anc is not None)
    map_rows = np.ascontiguousarray(map_rows, np.float32)
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    ev_in = np.ascontiguousarray(ev_in, np.uint8)
    n = len(x)
    L = map_rows.shape[2] if L is None else L
    stride = ev_in.shape[1]
    for v in (hit, miss, cmax):
        assert 1 <= int(v) <= 255
    assert np.isfinite(view_range) and view_range > 0 and stride >= L and 0 <= K <= 64
    assert np.isfinite(margin) and margin > 0 and len(T) in BINS
    hit, miss, cmax = int(hit), int(miss), int(cmax)
    with np.errstate(all="ignore"):
        range2 = F(view_range) * F(view_range)
    src = np.arange(n) if anc is None else np.asarray(anc, np.int64)
    c = ev_in[src][:, :L].astype(np.int64)
    a = np.asarray(assoc)[:n, :L].astype(np.int64)
    mx, my, pxx = map_rows[:n, 0, :L], map_rows[:n, 1, :L], map_rows[:n, 2, :L]
    px, py = x[:, None], y[:, None]
    seen = ~(pxx < 0)
    hit_now = a < K
    with np.errstate(all="ignore"):
        dx = mx - px
        dy = my - py
        t = dx * dx
        u = dy * dy
        r2 = t + u
        visible = r2 <= range2
    hid = hidden(T, margin, x, y, th, mx, my)[0] if L > 0 else np.zeros((n, 0), bool)
    due = seen & ~hit_now & visible
    miss_now = due & ~hid
    prune = miss_now & (c < miss)
    out = np.where(seen & hit_now, np.minimum(c + hit, cmax), c)
    out = np.where(miss_now & ~prune, c - miss, out)
    out = np.where(prune | ~seen, 0, out)
    map_out = map_rows.copy()
    for p in range(5):
        map_out[:n, p, :L] = np.where(prune, E.FRESH[p], map_rows[:n, p, :L])
    ev_out = ev_in[src].copy() if in_place else np.zeros((n, stride), np.uint8)
    ev_out[:, :L] = out.astype(np.uint8)
    stats = np.stack([prune.sum(axis=1), (seen & ~prune).sum(axis=1)], axis=1).astype(np.int32)
    spared = (due & hid).sum(axis=1).astype(np.int32)
    return map_out, ev_out, stats, spared


def frame_loop(world, scans, n, *, seed, sigma, meas_var, score_gain, dp, gate, new_gate, create, prune, sight=None, ess=0.0,
               refine=None, detect_params=None, detections=None, score=True):
    """_detect_spec.frame_loop with the sight table of frame f's scan built before its evidence stage: what a rows session with
    slam_pf_assoc_set, slam_pf_prune_set, slam_pf_detect_set and slam_pf_prune_sight_set does.  sight: (bins, margin), None (off:
    exactly _detect_spec.frame_loop), or a function of the frame number that returns either.  score = False: a zero scan-match
    score (a drive without a grid: the CPU behaviour test).
    -> one dict per frame as _detect_spec.frame_loop's, plus spared int32 [n] and table (None on a frame without sight)."""
    import oracle
    import _assoc_spec as A
    import _detect_spec as D
    import _refine_spec as R

    out = []
    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled = None, None, True
    ev = E.evidence_init(mp, prune[2])
    for f, (bx, by) in enumerate(scans):
        sg = sight(f) if callable(sight) else sight
        if detections is not None:
            zx, zy = detections(f)
        else:
            dzx, dzy, k, _ = D.detect(bx, by, **(detect_params or {}))
            zx, zy = dzx[:k].copy(), dzy[:k].copy()
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp, sigma, seed, f)
        if not score:
            sc = np.zeros(n, np.float32)
        elif refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], bx, by, x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)
        assoc, stats = A.associate(mp, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create)
        mp, ll = A.update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
        spared = T = None
        if sg:
            T = table(bx, by, sg[0])
            mp, ev, ev_stats, spared = evidence(mp, x, y, th, anc, assoc, len(zx), ev, *prune, T, sg[1])
        else:
            mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, len(zx), ev, *prune)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc], ev_raw=ev, ev_stats=ev_stats, det=(zx, zy), spared=spared, table=T))
    return out
