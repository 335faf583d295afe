"""The specification of the landmark merge ("Merging duplicate landmarks"; include/slam_hip.h:
slam_landmark_merge_dev, slam_pf_merge_set) in numpy float32, one rounded operation per line.  TEST INFRASTRUCTURE shared by
test_merge_spec_cpu.py, test_merge_behaviour_cpu.py and the GPU tests.  It uses numpy's float32 division, the cost of a pair from
tests/_assoc_spec.py, the operation order of tests/_aniso_spec.py: update_one for the fusion, and nothing of the package.

Two slots of one particle that hold the same pole were fed disjoint sets of detections (a detection updates exactly one landmark
of a particle), so given the particle's path they are independent estimates of one point and their product is the posterior.
The stage runs behind the frame's associating update (and its evidence stage), in place on the row the update wrote:

  roles     seen = !(P_xx < 0); ANCHOR = seen and a_l < K (matched or created this frame); FREE = seen and not a_l < K.  A table
            names a detection at most once, so a particle has at most K <= 64 anchors; of a table that does not, the anchors
            behind the 64th in ascending l take no part (they are neither anchor nor free).  Two anchors are never merged.
  choice 1  a free l walks the anchors w in ascending w: d = mu_l - mu_w, S = P_l + P_w, m = d^T S^-1 d (shared_pair + the
            association's cost); it keeps the cheapest (strict <, from +inf: the lowest w on ties, NaN never wins) and is a
            candidate iff 0 <= m <= merge_gate.
  choice 2  an anchor absorbs, of the candidates that chose it, the cheapest (the lowest l on ties; -0 counts as +0) — one per frame.
  fusion    fuse(): the general-covariance update of the anchor with mu_l as the observed point and P_l as the noise, no
            likelihood term.
  guard     refused (counted, nothing written) unless the five values are finite, P'_xx > 0, P'_yy > 0 and P'_xx P'_yy - P'_xy^2 > 0.
  result    anchor <- the five values; slot l <- (0, 0, -1, 0, 0); with evidence c_w' = min(c_w + c_l, cmax), c_l' = 0.
  stats     int32 [n][3] = merged, refused, seen after the stage.
"""
import numpy as np

import _assoc_spec as A

F = np.float32
FRESH = (F(0.0), F(0.0), F(-1.0), F(0.0), F(0.0))   # the five planes of a slot that was never used
MAX_ANCHORS = A.MAX_DETECTIONS


def roles(map_rows, assoc, K, L):
    """-> (seen, anchor, free) bool [n][L]; the anchors behind the 64th of a particle are neither."""
    seen = ~(map_rows[:, 2, :L] < 0)
    named = seen & (np.asarray(assoc)[:, :L].astype(np.int64) < K)
    anchor = named & (np.cumsum(named, axis=1) <= MAX_ANCHORS)
    return seen, anchor, seen & ~named


def shared_pair(lxx, lxy, lyy, wxx, wxy, wyy):
    """S^-1 of S = P_l + P_w -> (i00, i01, i11, idet): the operations of _aniso_spec.update_one (and of _assoc_aniso_spec.shared)
    with P_w as the prior and P_l as the noise."""
    a = wxx + lxx
    b = wxy + lxy
    cc = wyy + lyy
    t = a * cc
    u = b * b
    det = t - u
    idet = F(1.0) / det
    i00 = cc * idet
    i01 = (-b) * idet
    i11 = a * idet
    return i00, i01, i11, idet


def pair_cost(ml, mw):
    """m(l, w): ml, mw tuples of five float32 arrays (mu_x, mu_y, P_xx, P_xy, P_yy) that broadcast."""
    i00, i01, i11, _ = shared_pair(ml[2], ml[3], ml[4], mw[2], mw[3], mw[4])
    return A.cost((None, mw[0], mw[1], i00, i01, i11), ml[0], ml[1])   # dx = mu_l - mu_w


def fuse(ml, mw):
    """The absorbed landmark ml into the anchor mw -> (mu_x', mu_y', P_xx', P_xy', P_yy'): _aniso_spec.update_one with the
    observed point w = mu_l, R_w = P_l, detq = det P_l (float32, from P_l's three values), and without its likelihood term."""
    lx, ly, lxx, lxy, lyy = ml
    mx, my, pxx, pxy, pyy = mw
    i00, i01, i11, idet = shared_pair(lxx, lxy, lyy, pxx, pxy, pyy)
    dx = lx - mx
    dy = ly - my
    t = i00 * dx
    u = i01 * dy
    t0 = t + u
    t = i01 * dx
    u = i11 * dy
    t1 = t + u
    t = lxx * t0
    u = lxy * t1
    t = t + u
    o0 = lx - t
    t = lxy * t0
    u = lyy * t1
    t = t + u
    o1 = ly - t
    t = pxx * pyy
    u = pxy * pxy
    detp = t - u
    t = lxx * lyy
    u = lxy * lxy
    detl = t - u
    t = detp * lxx
    u = detl * pxx
    t = t + u
    o2 = idet * t
    t = detp * lxy
    u = detl * pxy
    t = t + u
    o3 = idet * t
    t = detp * lyy
    u = detl * pyy
    t = t + u
    o4 = idet * t
    return o0, o1, o2, o3, o4


def guard(o):
    """A fused landmark that may be written: finite, P_xx > 0, P_yy > 0, float32 determinant > 0."""
    o0, o1, o2, o3, o4 = o
    t = o2 * o4
    u = o3 * o3
    d = t - u
    fin = np.isfinite(o0) & np.isfinite(o1) & np.isfinite(o2) & np.isfinite(o3) & np.isfinite(o4)
    return fin & (o2 > 0) & (o4 > 0) & (d > 0)


def merge(map_rows, assoc, K, merge_gate, ev=None, cmax=None, L=None):
    """map_rows: float32 [n][5][plane_stride >= L], the rows AFTER the frame's update (and evidence stage); assoc: uint8 [n][>= L]
    the frame's table; K: the number of detections of the frame; ev (optional): uint8 [n][ev_stride >= L] with cmax in 1 .. 255.
    The columns from L on are never touched.  -> (map_out, ev_out or None, stats int32 [n][3] = merged, refused, seen after)."""
    map_rows = np.ascontiguousarray(map_rows, np.float32)
    n = map_rows.shape[0]
    L = map_rows.shape[2] if L is None else L
    gate = F(merge_gate)
    assert np.isfinite(gate) and gate > 0 and 0 <= K <= A.MAX_DETECTIONS
    if ev is not None:
        ev = np.ascontiguousarray(ev, np.uint8)
        assert 1 <= int(cmax) <= 255 and ev.shape[1] >= L
    out = map_rows.copy()
    ev_out = None if ev is None else ev.copy()
    stats = np.zeros((n, 3), np.int32)
    seen, anchor, free = roles(map_rows, assoc, K, L)
    stats[:, 2] = seen.sum(axis=1)
    count = anchor.sum(axis=1)
    if L == 0 or count.max(initial=0) == 0:
        return out, ev_out, stats
    rows = np.arange(n)
    planes = tuple(map_rows[:, p, :L] for p in range(5))
    # the anchors in ascending w: slot[i][j] = the j-th anchor of particle i
    slot = np.zeros((n, MAX_ANCHORS), np.int64)
    for i in np.flatnonzero(count):
        slot[i, :count[i]] = np.flatnonzero(anchor[i])
    nan = F(np.nan)
    ml = (np.where(free, planes[0], nan),) + planes[1:]   # a slot that is not free: NaN in its mean, every m NaN, never chosen
    # 1. the free landmark chooses
    best = np.full((n, L), np.inf, np.float32)
    bj = np.zeros((n, L), np.int64)
    with np.errstate(all="ignore"):
        for j in range(int(count.max())):
            has = (count > j)[:, None]
            mw = tuple(np.where(has, planes[p][rows, slot[:, j]][:, None], nan if p == 0 else F(1.0)) for p in range(5))
            m = pair_cost(ml, mw)
            take = m < best
            best = np.where(take, m, best)
            bj = np.where(take, j, bj)
    cand = free & (best >= 0) & (best <= gate)
    # 2. the anchor chooses, 3. fusion, guard and result — every pair reads the row as the stage found it
    for j in range(int(count.max())):
        mine = cand & (bj == j)
        for i in np.flatnonzero(mine.any(axis=1)):
            l = int(np.argmin(np.where(mine[i], best[i], np.inf)))   # the first minimum: the lowest l; -0 == +0
            w = int(slot[i, j])
            with np.errstate(all="ignore"):
                o = fuse(tuple(planes[p][i, l] for p in range(5)), tuple(planes[p][i, w] for p in range(5)))
                ok = bool(guard(o))
            if not ok:
                stats[i, 1] += 1
                continue
            for p in range(5):
                out[i, p, w] = o[p]
                out[i, p, l] = FRESH[p]
            if ev is not None:
                ev_out[i, w] = min(int(ev[i, w]) + int(ev[i, l]), int(cmax))
                ev_out[i, l] = 0
            stats[i, 0] += 1
    stats[:, 2] -= stats[:, 0]
    return out, ev_out, stats


def frame_loop(world, n, frames, *, seed, sigma, meas_var, score_gain, dp, detections, gate, new_gate, create, merge_gate,
               meas_cov=None, prune=None, ess=0.0, score=True):
    """_assoc_spec.frame_loop (meas_cov None) or _assoc_aniso_spec.frame_loop (meas_cov = (qxx, qxy, qyy)), with
    _evidence_spec.evidence behind the update where prune = (hit, miss, cmax, view_range), plus the stage above behind both on
    every frame with a detection hand-over: what a rows session does once slam_pf_merge_set was called.  merge_gate 0: off.
    -> one dict per frame as those loops', plus merge_stats (None on a frame without the stage)."""
    import oracle
    import _assoc_aniso_spec as AA
    import _evidence_spec as E

    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled, out = None, None, True, []
    ev = E.evidence_init(mp, prune[2]) if prune else None
    for f in range(frames):
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp(f) if callable(dp) else dp, sigma, seed, f)
        if score:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], world["bx"], world["by"], x, y, th)
        else:
            sc = np.zeros(n, np.float32)
        det = detections(f)
        assoc = stats = ev_stats = merge_stats = None
        if det is None:
            if anc is not None:
                mp = mp[anc]
                ev = ev[anc] if prune else ev
            ll = None
        else:
            zx, zy = det
            if meas_cov is None:
                assoc, stats = A.associate(mp, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create)
                mp, ll = A.update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
            else:
                assoc, stats = AA.associate(mp, x, y, th, anc, zx, zy, meas_cov, gate, new_gate, create)
                mp, ll = AA.update(mp, x, y, th, anc, assoc, zx, zy, meas_cov)
            if prune:
                mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, len(zx), ev, *prune)
            if merge_gate:
                mp, ev, merge_stats = merge(mp, assoc, len(zx), merge_gate, ev, prune[2] if prune else None)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if prune else None, ev_raw=ev if prune else None, ev_stats=ev_stats,
                        merge_stats=merge_stats))
    return out
