"""The specification of the landmark detector ("Detector"; include/slam_hip.h: slam_detect_scan_dev,
slam_pf_detect_set) in float32 numpy, one rounded operation per line, no fused multiply-add.  TEST INFRASTRUCTURE shared by
test_detect_spec_cpu.py, test_detect_behaviour_cpu.py and the GPU tests.  It uses nothing of the package.

The scan is P points in scan order (what fe_clean left: removed beams leave no hole, so the rule uses distances only).  A point
whose squared gap to its predecessor exceeds jump^2 BREAKS the scan; the points from one break up to the next are a SEGMENT.  A
segment of min_points .. max_points points, no wider than max_width, with nothing nearer close to either end (an occluder) and its
centroid within max_range is a DETECTION: its centroid, a sensor-frame point without identity.
"""
import numpy as np

F = np.float32
MAX_DETECTIONS = 64
MAX_POINTS = 64     # SLAM_DETECT_MAX_POINTS
MAX_BEAMS = 4096
DEFAULTS = dict(jump=0.3, guard=1.0, max_width=0.5, max_range=20.0, min_points=3, max_points=40, wrap=1)


def params(**kw):
    p = dict(DEFAULTS)
    p.update(kw)
    return p


def params_ok(p):
    fl = [np.float32(p[k]) for k in ("jump", "guard", "max_width", "max_range")]
    return (all(np.isfinite(v) and v > 0 for v in fl) and fl[1] >= fl[0] and
            1 <= int(p["min_points"]) <= int(p["max_points"]) <= MAX_POINTS and int(p["wrap"]) in (0, 1))


def detect(bx, by, **kw):
    """-> (zx float32 [64], zy float32 [64], ndet, stats int32 [4] = segments, accepted, written, 0); the entries from ndet on are
    0.  Keywords: the fields of slam_detect_params (defaults: slam_detect_params_default)."""
    p = params(**kw)
    assert params_ok(p)
    x, y = np.ascontiguousarray(bx, F), np.ascontiguousarray(by, F)
    P = len(x)
    assert len(y) == P and 0 <= P <= MAX_BEAMS
    wrap, minp, maxp = int(p["wrap"]), int(p["min_points"]), int(p["max_points"])
    zx, zy = np.zeros(MAX_DETECTIONS, F), np.zeros(MAX_DETECTIONS, F)
    if P == 0:
        return zx, zy, 0, np.zeros(4, np.int32)
    with np.errstate(all="ignore"):
        jump2 = F(p["jump"]) * F(p["jump"])
        guard2 = F(p["guard"]) * F(p["guard"])
        width2 = F(p["max_width"]) * F(p["max_width"])
        range2 = F(p["max_range"]) * F(p["max_range"])
        # 1. per point
        xx = x * x
        yy = y * y
        r2 = xx + yy
        dx = x - np.roll(x, 1)
        dy = y - np.roll(y, 1)
        dx2 = dx * dx
        dy2 = dy * dy
        g = dx2 + dy2
        if not wrap:
            g[0] = F(np.inf)
        brk = ~(g <= jump2)
    starts = np.flatnonzero(brk)
    accepted = written = 0
    for s, f in enumerate(starts):
        f = int(f)
        # 2. the segment: up to but excluding the next break (cyclic with wrap; the only break: the whole scan)
        if s + 1 < len(starts):
            m = int(starts[s + 1]) - f
        elif wrap:
            m = int(starts[0]) + P - f
        else:
            m = P - f
        if not wrap and (f == 0 or f + m - 1 == P - 1):
            continue                                  # cut by the field of view
        if not (minp <= m <= maxp):                   # (a)
            continue
        idx = (f + np.arange(m)) % P
        e, pp, q = int(idx[-1]), (f - 1) % P, (f + m) % P
        with np.errstate(all="ignore"):
            wdx = x[e] - x[f]                         # (b)
            wdy = y[e] - y[f]
            wdx2 = wdx * wdx
            wdy2 = wdy * wdy
            w2 = wdx2 + wdy2
            if not (w2 <= width2):
                continue
            if g[f] <= guard2 and r2[pp] < r2[f]:     # (c) occluded on the left
                continue
            if g[q] <= guard2 and r2[q] < r2[e]:      # ... on the right
                continue
            sx, sy = x[f], y[f]                       # (d) the centroid, summed in segment order
            for b in idx[1:]:
                sx = sx + x[b]
                sy = sy + y[b]
            cx = sx / F(m)
            cy = sy / F(m)
            cxx = cx * cx
            cyy = cy * cy
            c2 = cxx + cyy
            if not (c2 <= range2):
                continue
        if written < MAX_DETECTIONS:                  # 4. ascending f, the first 64
            zx[written], zy[written] = cx, cy
            written += 1
        accepted += 1
    return zx, zy, written, np.array([len(starts), accepted, written, 0], np.int32)


# ------------------------------------------------------------------ scenes for the behaviour and session tests
def raycast(pose, poles, rho, half, nbeams=360, noise=None, angles=None):
    """Ranges of `nbeams` beams from pose (x, y, th) in a square room [-half, half]^2 with circular poles (centres [k][2], radius
    rho), in float64; the pose in the project's convention (a sensor-frame point is z = R(theta) (w - t): the beam at sensor angle
    a points along a - theta in the world); noise: a Generator -> range noise of 1 cm; angles: the beams' sensor angles instead of
    a full circle of nbeams.
    -> (bx, by float32 sensor-frame points, hit int [nbeams]: the pole a beam ends on, -1 = a wall, the noise added [nbeams])."""
    px, py, th = (float(v) for v in pose)
    ang = -np.pi + 2 * np.pi * np.arange(nbeams) / nbeams if angles is None else np.asarray(angles, np.float64)
    nbeams = len(ang)
    c, s = np.cos(ang - th), np.sin(ang - th)
    with np.errstate(divide="ignore"):
        tx = np.where(c > 0, (half - px) / c, np.where(c < 0, (-half - px) / c, np.inf))
        ty = np.where(s > 0, (half - py) / s, np.where(s < 0, (-half - py) / s, np.inf))
    rng_ = np.minimum(tx, ty)
    hit = np.full(nbeams, -1)
    for k, (cx, cy) in enumerate(np.asarray(poles, np.float64)):
        ox, oy = px - cx, py - cy
        bq = ox * c + oy * s
        disc = bq * bq - (ox * ox + oy * oy - rho * rho)
        t = -bq - np.sqrt(np.where(disc >= 0, disc, np.nan))
        ok = (disc >= 0) & (t > 0) & (t < rng_)
        rng_ = np.where(ok, t, rng_)
        hit = np.where(ok, k, hit)
    added = 0.01 * noise.standard_normal(nbeams) if noise is not None else np.zeros(nbeams)
    rng_ = rng_ + added
    return (rng_ * np.cos(ang)).astype(F), (rng_ * np.sin(ang)).astype(F), hit, added


def frame_loop(world, scans, n, *, seed, sigma, meas_var, score_gain, dp, gate, new_gate, create, prune=None, ess=0.0, refine=None,
               detect_params=None, detections=None):
    """What a rows session with slam_pf_assoc_set (+ slam_pf_prune_set) and slam_pf_detect_set does over the frames scans[f] =
    (bx, by): _evidence_spec.frame_loop with the frame's own scan and detections(f) = detect(scan f).  `detections`: a function of
    the frame number that overrides the detector (the same loop fed ideal detections).
    -> one dict per frame as _evidence_spec.frame_loop's, plus det = (zx, zy) of the frame."""
    import oracle
    import _assoc_spec as A
    import _evidence_spec as E
    import _refine_spec as R

    out = []
    x, y, th, mp = (np.ascontiguousarray(world[k][:n]) for k in ("x", "y", "th", "mp"))
    fq = oracle.ess_frac_q16(ess)
    anc, carry, prev_resampled = None, None, True
    ev = E.evidence_init(mp, prune[2]) if prune else None
    for f, (bx, by) in enumerate(scans):
        if detections is not None:
            zx, zy = detections(f)
        else:
            dzx, dzy, k, _ = detect(bx, by, **(detect_params or {}))
            zx, zy = dzx[:k].copy(), dzy[:k].copy()
        x, y, th = oracle.motion_sample(x, y, th, anc, n, 0, dp, sigma, seed, f)
        if refine:
            x, y, th, sc, _ = R.refine(oracle, world["meta"], world["edt"], bx, by, x, y, th, *refine)
        else:
            sc, _ = oracle.score_poses_det(world["meta"], world["edt"], bx, by, x, y, th)
        assoc, stats = A.associate(mp, x, y, th, anc, zx, zy, meas_var, gate, new_gate, create)
        mp, ll = A.update(mp, x, y, th, anc, assoc, zx, zy, meas_var)
        ev_stats = None
        if prune:
            mp, ev, ev_stats = E.evidence(mp, x, y, anc, assoc, len(zx), ev, *prune)
        logw, m = oracle.logweight_carry(sc, ll, score_gain, None if prev_resampled else carry)
        wq, _ = oracle.quantise_weights(logw, m)
        s16, q16 = oracle.ess_terms(wq)
        prev_resampled = oracle.ess_resample(s16, q16, n, fq) if fq else True
        carry = oracle.weight_carry(logw, m)
        anc = oracle.resample(wq, seed, f) if prev_resampled else np.arange(n, dtype=np.int32)
        out.append(dict(pose=np.stack([x[anc], y[anc], th[anc]]), map=mp[anc], logw=logw, anc=anc, resampled=prev_resampled,
                        assoc=assoc, stats=stats, ev=ev[anc] if prune else None, ev_raw=ev if prune else None, ev_stats=ev_stats,
                        det=(zx, zy)))
    return out
