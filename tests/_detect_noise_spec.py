"""The specification of the detector's NOISE MODEL (include/slam_hip.h: slam_detect_scan_noise_dev,
slam_pf_detect_noise_set) in float32 numpy, one rounded operation per line, no fused multiply-add.  TEST INFRASTRUCTURE shared
by test_detect_noise_spec_cpu.py and the GPU tests.  It uses nothing of the package; tests/_detect_fit_spec.py stays the
specification of what a segment puts out and is only run here.

Every point (zx, zy) that _detect_fit_spec.detect_fit accepts (with or without a fit: it passed its range test) gets
    Q = a u u^T + b v v^T,   u = (zx, zy) / |z| its line of sight, v normal to u,   a = range_var,   b = bearing_var |z|^2 + lateral_var.
A point with r2 == 0, or whose Q fails the rule of _aniso_spec.valid_cov (finite, qxx > 0, qyy > 0, float32 determinant > 0:
cancellation at extreme a : b), is NO detection.  The cap at MAX_DETECTIONS applies AFTER this rule: the first 64 of what is left,
by ascending start."""
import types

import numpy as np

import _aniso_spec as S
import _detect_fit_spec as DF
import _detect_spec as D

F = np.float32
MAX_DETECTIONS = D.MAX_DETECTIONS

# _detect_fit_spec.detect_fit itself, word for word, with its cap lifted to the number of points a scan can hold (a segment has at
# least one): everything it accepts, by ascending start
_accept_all = types.FunctionType(DF.detect_fit.__code__, dict(DF.__dict__, MAX_DETECTIONS=D.MAX_BEAMS), "detect_fit_uncapped",
                                 DF.detect_fit.__defaults__)
_accept_all.__kwdefaults__ = DF.detect_fit.__kwdefaults__


def noise_ok(noise):
    """range_var finite and > 0; bearing_var and lateral_var finite and >= 0; bearing_var + lateral_var > 0 — on the float32 values."""
    with np.errstate(all="ignore"):
        a, b, c = (F(v) for v in noise)
        return bool(np.isfinite(a) and a > 0 and np.isfinite(b) and b >= 0 and np.isfinite(c) and c >= 0 and F(b + c) > 0)


def cov_of(zx, zy, noise):
    """One detection (float32 scalars or arrays) -> (qxx, qxy, qyy, ok): ok False where r2 == 0 or Q fails the validity rule."""
    zx, zy = np.asarray(zx, F), np.asarray(zy, F)
    rv, bv, lv = (F(v) for v in noise)
    with np.errstate(all="ignore"):
        zxx = zx * zx
        zyy = zy * zy
        r2 = zxx + zyy
        rho = np.sqrt(r2)
        ux = zx / rho
        uy = zy / rho
        a = rv
        t = bv * r2
        b = t + lv
        uxx = ux * ux
        uyy = uy * uy
        uxy = ux * uy
        x0 = a * uxx
        x1 = b * uyy
        qxx = x0 + x1
        d = a - b
        qxy = d * uxy
        y0 = a * uyy
        y1 = b * uxx
        qyy = y0 + y1
        d0 = qxx * qyy                      # the validity rule: _aniso_spec.det_q's three operations
        d1 = qxy * qxy
        detq = d0 - d1
        ok = (r2 > 0) & np.isfinite(qxx) & np.isfinite(qxy) & np.isfinite(qyy) & (qxx > 0) & (qyy > 0) & (detq > 0)
    return qxx.astype(F), qxy.astype(F), qyy.astype(F), ok


def detect_noise(bx, by, fit=None, noise=None, **kw):
    """noise None: exactly _detect_fit_spec.detect_fit -> (zx, zy, ndet, stats [4]).
    noise = (range_var, bearing_var, lateral_var) -> (zx [64], zy [64], (qxx [64], qxy [64], qyy [64]), ndet, stats int32 [6] =
    segments, accepted, written, rejected by the shape test, dropped by the noise rule, 0); accepted and written count what passed
    the noise rule; the entries from ndet on are 0."""
    if noise is None:
        return DF.detect_fit(bx, by, fit, **kw)
    assert noise_ok(noise)
    ax, ay, n_all, st = _accept_all(bx, by, fit, **kw)
    qxx, qxy, qyy, ok = cov_of(ax[:n_all], ay[:n_all], noise)
    for k in range(n_all):                  # (the rule, restated on the one detection: the same verdict)
        assert bool(ok[k]) == (bool(ax[k] * ax[k] + ay[k] * ay[k] > 0) and S.valid_cov((qxx[k], qxy[k], qyy[k])))
    keep = np.flatnonzero(ok)
    written = min(len(keep), MAX_DETECTIONS)
    out = [np.zeros(MAX_DETECTIONS, F) for _ in range(5)]
    for o, v in zip(out, (ax[:n_all], ay[:n_all], qxx, qxy, qyy)):
        o[:written] = v[keep[:written]]
    stats = np.array([st[0], len(keep), written, st[3], n_all - len(keep), 0], np.int32)
    return out[0], out[1], (out[2], out[3], out[4]), written, stats
