"""The specification of the detector's noise model (tests/_detect_noise_spec.py) by itself: Q_k against float64, its axes, the
two drops, and noise = None.  No GPU.

Q AGAINST FLOAT64 (u = 2^-24; the reference takes the same float32 z and the same float32 model values).  r2 = zx^2 + zy^2 is a
sum of two rounded positive products: relative error 2 u.  rho = sqrt(r2): u + u / 2.  ux = zx / rho: another u / 2, so ux and
uy carry 2.5 u each and their three products 5.5 u (rounded: 6 u).  b = bearing_var r2 + lateral_var: the product 3 u, the sum of
positives u more: 4 u.  qxx = a uxx + b uyy is a sum of positives: a uxx carries 7 u, b uyy 11 u, the sum u more — at most 12 u of
qxx <= 12 u max(a, b); qyy likewise.  qxy = (a - b) uxy: a - b carries 4 u b + u |a - b| in absolute terms, uxy 6 u, the product
u, and |uxy| <= 1 / 2: |dqxy| <= (4 u b + 8 u |a - b|) / 2 <= 6 u max(a, b).  First order throughout; the second-order terms
are below u^2 * 100: one more u covers them.  Every entry: |Q - Q_64| <= 13 u max(a, b)."""
import numpy as np
import pytest

import _aniso_spec as A
import _detect_fit_spec as DF
import _detect_noise_spec as DN
import _detect_scenes as S
import _f64_pf as F64

U = F64.U
MODELS = ((1e-4, 1.5625e-4, 1e-4), (4e-6, 1e-4, 0.0), (1e-2, 0.0, 1e-2), (1e-6, 1e-2, 0.0))
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def points(n=20000, seed=1):
    """Detections all round the sensor from 1 cm to 1 km, the axes and the diagonals among them."""
    rng = np.random.default_rng(seed)
    r = 10.0 ** rng.uniform(-2, 3, n)
    b = rng.uniform(-np.pi, np.pi, n)
    b[:8] = np.arange(8) * np.pi / 4
    return (r * np.cos(b)).astype(np.float32), (r * np.sin(b)).astype(np.float32)


def q64(zx, zy, noise):
    zx, zy = zx.astype(np.float64), zy.astype(np.float64)
    rv, bv, lv = (float(np.float32(v)) for v in noise)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = rv, bv * r2 + lv
    return a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux, a, b, ux, uy


@pytest.mark.parametrize("noise", MODELS)
def test_q_within_its_bound_of_float64_and_its_axes_lie_along_and_across_the_line_of_sight(noise):
    zx, zy = points()
    qxx, qxy, qyy, ok = DN.cov_of(zx, zy, noise)
    rxx, rxy, ryy, a, b, ux, uy = q64(zx, zy, noise)
    bound = 13 * U * np.maximum(a, b)
    worst = max(float(np.max(np.abs(g - r) / bound)) for g, r in ((qxx, rxx), (qxy, rxy), (qyy, ryy)))
    print(f"{noise}: max |Q - Q_64| / bound {worst:.3g}; valid {ok.mean():.4f}")
    assert worst <= 1.0
    # Q u = a u and Q v = b v with v = (-uy, ux): each component is two entries times a unit vector's components — twice the bound
    g = [v.astype(np.float64) for v in (qxx, qxy, qyy)]
    along = np.hypot(g[0] * ux + g[1] * uy - a * ux, g[1] * ux + g[2] * uy - a * uy)
    across = np.hypot(-g[0] * uy + g[1] * ux + b * uy, -g[1] * uy + g[2] * ux - b * ux)
    assert np.all(along <= 2 * np.sqrt(2) * bound) and np.all(across <= 2 * np.sqrt(2) * bound)
    # where the rule passes, the matrix is what the per-detection stages accept
    for k in np.flatnonzero(ok)[:200]:
        assert A.valid_cov((qxx[k], qxy[k], qyy[k]))
    assert ok[:8].all() or noise[0] < 1e-5                           # (the axes and diagonals at moderate a : b)


def test_the_two_drops():
    # r2 == 0: the point on the sensor, and one whose squares underflow
    for z in ((0.0, 0.0), (1e-30, -1e-30)):
        assert not DN.cov_of(np.float32(z[0]), np.float32(z[1]), MODELS[0])[3]
    # cancellation in det Q at extreme a : b off the axes: qxx qyy and qxy^2 agree to the last bit, the float32 determinant is not > 0
    noise = (1e-12, 1.0, 0.0)
    zx, zy = points(4000, 2)
    qxx, qxy, qyy, ok = DN.cov_of(zx, zy, noise)
    assert 0 < (~ok).sum() < len(ok)
    bad = np.flatnonzero(~ok)
    assert all(not A.valid_cov((qxx[k], qxy[k], qyy[k])) for k in bad[:200])
    assert ok[[0, 2, 4, 6]].all()                                     # on the axes qxy is tiny and nothing cancels
    # in the detector: the dropped ones are counted, and the cap applies to what is left
    bx, by, kw = S.pole_field(4096, 4196)
    plain = DF.detect_fit(bx, by, (0.3, 0.0), **kw)
    assert plain[3][1] > 64
    zx, zy, q, ndet, st = DN.detect_noise(bx, by, (0.3, 0.0), noise, **kw)
    assert st[4] > 0 and st[1] + st[4] == plain[3][1] and st[2] == ndet == min(st[1], 64) and st[5] == 0
    assert st[0] == plain[3][0] and st[3] == plain[3][3]
    assert not np.array_equal(bits(zx), bits(plain[0]))               # a dropped one among the first 64 lets a later one in
    assert all(A.valid_cov((q[0][k], q[1][k], q[2][k])) for k in range(ndet))


@pytest.mark.parametrize("fit", [None, (0.1, 0.0), (0.3, 0.0)])
def test_noise_none_is_the_fit_spec_and_a_model_changes_nothing_but_q(fit):
    for P in (360, 4096):
        bx, by, kw = S.pole_field(P, 100 + P)
        want = DF.detect_fit(bx, by, fit, **kw)
        got = DN.detect_noise(bx, by, fit, None, **kw)
        assert all(np.array_equal(bits(np.asarray(g)), bits(np.asarray(w))) for g, w in zip(got, want))
        zx, zy, q, ndet, st = DN.detect_noise(bx, by, fit, MODELS[0], **kw)   # a model that drops nothing: the same detections
        assert st[4] == 0 and ndet == want[2] and np.array_equal(st[:4], want[3])
        assert np.array_equal(bits(zx), bits(want[0])) and np.array_equal(bits(zy), bits(want[1]))
        assert not any(bits(v[ndet:]).any() for v in q)
    for bad in ((0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, -1.0, 2.0), (float("nan"), 1.0, 0.0), (1.0, float("inf"), 0.0)):
        assert not DN.noise_ok(bad)
    assert DN.noise_ok((1e-4, 0.0, 1e-4)) and DN.noise_ok((1e-4, 1e-4, 0.0))
