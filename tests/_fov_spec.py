"""The specification of the evidence stage's field of view ("Field of view"; include/slam_hip.h:
slam_fov_bound, slam_landmark_evidence_fov_dev, slam_pf_prune_fov_set) in float32 numpy, one rounded operation per line, no fused
multiply-add.  TEST INFRASTRUCTURE shared by test_fov_spec_cpu.py, test_fov_behaviour_cpu.py and the GPU tests.  It reuses
tests/_sight_spec.py and tests/_evidence_spec.py, changes neither, and uses nothing of the package.

The evidence of tests/_evidence_spec.py and tests/_sight_spec.py treats the sensor as a full circle.  Here a landmark that is due a
miss but whose direction in the sensor frame lies OUTSIDE the arc [lo, hi] of the diamond angle takes no miss and keeps its counter
(a hit still counts, whatever the direction).  lo > hi is the arc that wraps through p = 4 = 0: the ordinary one for a sensor with
a blind sector behind it, whose blind sector straddles p = 2.
"""
import numpy as np

import _evidence_spec as E
import _sight_spec as S

F = np.float32
ALL = (F(0.0), F(4.0))   # everything in view


def diamond(x, y):
    """-> (p float32 in [0, 4], has bool): the diamond angle of the sensor-frame points (x, y) — the p of _sight_spec.bin_of before
    it is scaled to a bin; has = False: the point has none (the origin, a point that is not finite; p = 0 there)."""
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
    return p, has


def bound(angle):
    """The diamond angle of the direction `angle` (radians, float64 cosine and sine rounded to float32) -> float32."""
    a = np.asarray(angle, np.float64)
    return diamond(np.cos(a).astype(F), np.sin(a).astype(F))[0]


def bounds_ok(lo, hi):
    return all(0.0 <= float(v) <= 4.0 for v in (lo, hi))   # (NaN fails)


def in_view(p, has, lo, hi):
    """A bound itself is in view; a point without a diamond angle is in view."""
    lo, hi = F(lo), F(hi)
    inside = ((p >= lo) & (p <= hi)) if lo <= hi else ((p >= lo) | (p <= hi))
    return ~has | inside


def sensor_frame(px, py, th, mx, my):
    """px, py, th [n]; mx, my [n][L] -> (zx, zy) = R(theta)(w - t), the operations of _sight_spec.hidden in their order."""
    import oracle

    px, py, th = (np.ascontiguousarray(a, F).reshape(-1, 1) for a in (px, py, th))
    mx, my = np.asarray(mx, F), np.asarray(my, F)
    s, c = oracle.det_sincos(th.ravel())
    s, c = s.reshape(-1, 1), c.reshape(-1, 1)
    with np.errstate(all="ignore"):
        dx = mx - px
        dy = my - py
        a = c * dx
        b = s * dy
        zx = a - b
        a = s * dx
        b = c * dy
        zy = a + b
    return zx, zy


def evidence(map_rows, x, y, th, anc, assoc, K, ev_in, hit, miss, cmax, view_range, lo, hi, T=None, margin=None, L=None, in_place=False):
    """_evidence_spec.evidence (T None) or _sight_spec.evidence (T: the sight table, margin > 0) with
    miss_now = due & in_view & ~hidden, due = seen & ~hit_now & visible; hidden counts only where due & in_view.
    -> (map_out, ev_out, stats int32 [n][2], spared int32 [n], outside int32 [n] = landmarks with due & ~in_view)."""
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
    assert bounds_ok(lo, hi)
    if T is not None:
        assert np.isfinite(margin) and margin > 0 and len(T) in S.BINS
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
    due = seen & ~hit_now & visible
    if L > 0:
        zx, zy = sensor_frame(x, y, th, mx, my)
        p, has = diamond(zx, zy)
        view = in_view(p, has, lo, hi)
    else:
        view = np.ones((n, 0), bool)
    outside_now = due & ~view
    hid = np.zeros((n, L), bool)
    if T is not None and L > 0:
        hid = S.hidden(T, margin, x, y, th, mx, my)[0] & due & view
    miss_now = due & view & ~hid
    prune = miss_now & (c < miss)
    out = np.where(seen & hit_now, np.minimum(c + hit, cmax), c)
    out = np.where(miss_now & ~prune, c - miss, out)
    out = np.where(prune | ~seen, 0, out)
    map_out = map_rows.copy()
    for pl in range(5):
        map_out[:n, pl, :L] = np.where(prune, E.FRESH[pl], map_rows[:n, pl, :L])
    ev_out = ev_in[src].copy() if in_place else np.zeros((n, stride), np.uint8)
    ev_out[:, :L] = out.astype(np.uint8)
    stats = np.stack([prune.sum(axis=1), (seen & ~prune).sum(axis=1)], axis=1).astype(np.int32)
    spared = hid.sum(axis=1).astype(np.int32)
    outside = outside_now.sum(axis=1).astype(np.int32)
    return map_out, ev_out, stats, spared, outside


def frame_loop(world, scans, n, *, seed, sigma, meas_var, score_gain, dp, gate, new_gate, create, prune, fov=None, sight=None, ess=0.0,
               refine=None, detect_params=None, detections=None, score=True):
    """_sight_spec.frame_loop with the field of view: what a rows session with slam_pf_assoc_set, slam_pf_prune_set,
    slam_pf_detect_set, slam_pf_prune_fov_set (and slam_pf_prune_sight_set) does.  fov: (lo, hi), None (off: exactly
    _sight_spec.frame_loop), or a function of the frame number that returns either; sight as in _sight_spec.frame_loop.
    -> one dict per frame as _sight_spec.frame_loop's, plus outside int32 [n] (None on a frame without the field of view)."""
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
        fv = fov(f) if callable(fov) else fov
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
        spared = outside = None
        T = S.table(bx, by, sg[0]) if sg else None
        if fv:
            mp, ev, ev_stats, spared, outside = evidence(mp, x, y, th, anc, assoc, len(zx), ev, *prune, fv[0], fv[1], T,
                                                         sg[1] if sg else None)
            spared = spared if sg else None
        elif sg:
            mp, ev, ev_stats, spared = S.evidence(mp, x, y, th, anc, assoc, len(zx), ev, *prune, T, sg[1])
        else:
            mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, len(zx), ev, *prune)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc], ev_raw=ev, ev_stats=ev_stats, det=(zx, zy), spared=spared, table=T,
                        outside=outside))
    return out
