"""The specification of the FITTED landmark detector ("Detector, fitted"; include/slam_hip.h:
slam_detect_scan_fit_dev, slam_pf_detect_fit_set) in float32 numpy, one rounded operation per line, no fused multiply-add.  TEST
INFRASTRUCTURE shared by test_detect_fit_spec_cpu.py, test_detect_fit_behaviour_cpu.py and the GPU tests.  It uses nothing of the
package; tests/_detect_spec.py stays the specification of the centroid detector and is only read here (its constants, its
parameter check).

Steps 1 to 3(d) are _detect_spec.detect's: the breaks, the segments, the point count, the width, the occlusion tests, the centroid
c = (cx, cy) and c2 = cx*cx + cy*cy <= range2.  A pole has a known nominal radius rho.  With s2 the mean squared distance of the
segment's m points to their centroid and C the circle's centre, sum (p_i - c) = 0 gives mean |p_i - C|^2 = s2 + |c - C|^2; for
points on the circle the left side is rho^2, so the centre lies sqrt(rho^2 - s2) from the centroid — along the line of sight through
c, by the symmetry of the visible arc.  A segment that is more spread out than a circle of radius rho can be (s2 > rho^2 + tol^2)
is no pole: the shape test."""
import numpy as np

import _detect_spec as D

F = np.float32
MAX_DETECTIONS = D.MAX_DETECTIONS
FIT_DEFAULT = (0.1, 0.0)    # slam_detect_fit_default


def fit_ok(fit):
    """radius finite and > 0, spread_tol finite and >= 0, tested on the float32 values."""
    with np.errstate(all="ignore"):
        radius, tol = F(fit[0]), F(fit[1])
    return bool(np.isfinite(radius) and radius > 0 and np.isfinite(tol) and tol >= 0)


def detect_fit(bx, by, fit=None, **kw):
    """-> (zx float32 [64], zy float32 [64], ndet, stats int32 [4] = segments, accepted, written, rejected by the shape test); the
    entries from ndet on are 0.  fit: None (the centroid: exactly _detect_spec.detect) or (radius, spread_tol).  Keywords: the
    fields of slam_detect_params."""
    p = D.params(**kw)
    assert D.params_ok(p) and (fit is None or fit_ok(fit))
    x, y = np.ascontiguousarray(bx, F), np.ascontiguousarray(by, F)
    P = len(x)
    assert len(y) == P and 0 <= P <= D.MAX_BEAMS
    wrap, minp, maxp = int(p["wrap"]), int(p["min_points"]), int(p["max_points"])
    zx, zy = np.zeros(MAX_DETECTIONS, F), np.zeros(MAX_DETECTIONS, F)
    if P == 0:
        return zx, zy, 0, np.zeros(4, np.int32)
    with np.errstate(all="ignore"):
        jump2 = F(p["jump"]) * F(p["jump"])
        guard2 = F(p["guard"]) * F(p["guard"])
        width2 = F(p["max_width"]) * F(p["max_width"])
        range2 = F(p["max_range"]) * F(p["max_range"])
        if fit is not None:
            rho2 = F(fit[0]) * F(fit[0])
            tol2 = F(fit[1]) * F(fit[1])
            lim = rho2 + tol2
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
    accepted = written = shape = 0
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
            ox, oy = cx, cy                           # what the segment puts out: without a fit its centroid
            if fit is not None:
                qq = F(0)                             # (e) the spread about the centroid, summed in segment order
                for b in idx:
                    du = x[b] - cx
                    dv = y[b] - cy
                    du2 = du * du
                    dv2 = dv * dv
                    e2 = du2 + dv2
                    qq = qq + e2
                s2 = qq / F(m)
                if not (s2 <= lim) or not (c2 > 0):   # not round enough for a pole / the centroid on the sensor: no direction
                    shape += 1
                    continue
                t = rho2 - s2                         # (f) the centre: sqrt(rho2 - s2) behind the centroid on its line of sight
                t = t if t > 0 else F(0)
                d = np.sqrt(t)
                n = np.sqrt(c2)
                ux = cx / n
                uy = cy / n
                fx = d * ux
                fy = d * uy
                ox = cx + fx
                oy = cy + fy
                oxx = ox * ox
                oyy = oy * oy
                o2 = oxx + oyy
                if not (o2 <= range2):
                    continue
        if written < MAX_DETECTIONS:                  # 4. ascending f, the first 64
            zx[written], zy[written] = ox, oy
            written += 1
        accepted += 1
    return zx, zy, written, np.array([len(starts), accepted, written, shape], np.int32)
