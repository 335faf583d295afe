"""The fitted detector's specification (tests/_detect_fit_spec.py): without a fit it IS tests/_detect_spec.py's detector, on every
scan the centroid detector's tests use; each edge of the fit sits where tests/_detect_fit_scenes.py names it; and the derivation —
points exactly on a circle, sampled symmetrically about the line of sight, give the circle's centre up to float32 rounding.  No GPU."""
import numpy as np
import pytest

import _detect_fit_scenes as FS
import _detect_fit_spec as DF
import _detect_scenes as S
import _detect_spec as D

F = np.float32
SCENES = S.scenarios()
FIT_SCENES = FS.scenarios()
U = 2.0 ** -24          # float32 unit roundoff


def same(a, b):
    return (np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)) and
            a[2] == b[2] and np.array_equal(a[3], b[3]) and a[3].dtype == b[3].dtype)


@pytest.mark.parametrize("name", sorted(SCENES))
def test_without_a_fit_it_is_the_centroid_detector_on_the_scenarios(name):
    bx, by, kw, _ = SCENES[name]
    assert same(DF.detect_fit(bx, by, None, **kw), D.detect(bx, by, **kw))
    assert same(DF.detect_fit(bx, by, **kw), D.detect(bx, by, **kw))


def test_without_a_fit_it_is_the_centroid_detector_on_fields_and_rooms():
    for P in (0, 1, 2, 63, 64, 65, 360, 1024, 4096):
        for wrap in (1, 0):
            bx, by, kw = S.pole_field(P, 100 + P)
            kw = dict(kw, wrap=wrap)
            assert same(DF.detect_fit(bx, by, None, **kw), D.detect(bx, by, **kw)), (P, wrap)
    rng = np.random.default_rng(3)
    ang = np.deg2rad(30.0 * np.arange(12) + rng.uniform(-5, 5, 12))
    rad = rng.uniform(2.5, 4.5, 12)
    poles = np.stack([rad * np.cos(ang), rad * np.sin(ang)], 1)
    for k, pose in enumerate([(0.0, 0.0, 0.0), (0.4, -0.3, 0.2), (-0.5, 0.2, -0.4), (0.3, 0.5, 1.0), (-0.2, -0.6, 2.5)]):
        bx, by, _, _ = D.raycast(pose, poles, 0.1, 6.0, 360, noise=np.random.default_rng(k) if k % 2 else None)
        assert same(DF.detect_fit(bx, by), D.detect(bx, by))
        assert D.detect(bx, by)[2] >= 8


@pytest.mark.parametrize("name", sorted(FIT_SCENES))
def test_fit_scenario(name):
    bx, by, kw, fit, want = FIT_SCENES[name]
    zx, zy, ndet, stats = DF.detect_fit(bx, by, fit, **kw)
    assert stats.tolist() == want, name
    assert ndet == stats[2] == min(stats[1], DF.MAX_DETECTIONS)
    assert np.isfinite(zx).all() and np.isfinite(zy).all()
    assert not zx[ndet:].any() and not zy[ndet:].any()
    # the segments, and what the centroid detector makes of them, are the centroid detector's
    base = D.detect(bx, by, **kw)
    assert stats[0] == base[3][0] and stats[1] + stats[3] <= base[3][1]


def test_the_edges_sit_where_the_scenarios_say():
    H, X = FS.H, FS.X
    # s2 == lim exactly: accepted, and with rho2 - s2 == 0 the detection is the centroid
    bx, by, kw, fit, _ = FIT_SCENES["spread_equal"]
    zx, zy, ndet, _ = DF.detect_fit(bx, by, fit, **kw)
    assert ndet == 1 and zx[0] == X and zy[0] == F(0)
    du = bx[1] - X
    assert du * du == F(fit[0]) * F(fit[0]) == H * H                       # s2 = (H*H + H*H) / 2 = lim, every step exact
    # one ulp above: the pair's spread is the next float32
    bx, by, kw, fit, _ = FIT_SCENES["spread_above"]
    du, dv = bx[1] - X, by[1] - F(0)
    assert (by[1] + by[2]) / F(2) == F(0) and du * du + dv * dv == np.nextafter(H * H, F(np.inf))
    assert D.detect(bx, by, **kw)[2] == 1                                   # the centroid detector takes it
    # the same with a tolerance: s2 == rho2 + tol2; rho2 - s2 < 0 is clamped: the centroid
    bx, by, kw, fit, _ = FIT_SCENES["spread_equal_tol"]
    du, dv = bx[1] - X, by[1] - F(0)
    assert du * du + dv * dv == F(fit[0]) * F(fit[0]) + F(fit[1]) * F(fit[1])
    zx, zy, ndet, _ = DF.detect_fit(bx, by, fit, **kw)
    assert ndet == 1 and zx[0] == X and zy[0] == F(0)
    # clamped inside the tolerance: rho2 = H*H / 4 < s2 = H*H <= lim
    bx, by, kw, fit, _ = FIT_SCENES["clamped"]
    assert F(fit[0]) * F(fit[0]) < H * H <= F(fit[0]) * F(fit[0]) + F(fit[1]) * F(fit[1])
    zx, zy, ndet, _ = DF.detect_fit(bx, by, fit, **kw)
    assert ndet == 1 and zx[0] == X and zy[0] == F(0)
    # an ordinary fit: sqrt(rho2 - s2) behind the centroid, on the axis
    bx, by, kw, fit, _ = FIT_SCENES["behind"]
    zx, zy, ndet, _ = DF.detect_fit(bx, by, fit, **kw)
    d = np.sqrt(F(0.0625) - H * H)
    assert ndet == 1 and zx[0] == X + d * (X / np.sqrt(X * X)) and zy[0] == F(0) and zx[0] > X + F(0.2)
    # c2 == 0
    bx, by, kw, fit, _ = FIT_SCENES["on_the_sensor"]
    c = D.detect(bx, by, **kw)
    assert c[2] == 1 and c[0][0] == 0 and c[1][0] == 0
    # the range test of the fitted point
    bx, by, kw, fit, _ = FIT_SCENES["fitted_out_of_range"]
    assert D.detect(bx, by, **kw)[2] == 1
    zx, _, ndet, _ = DF.detect_fit(bx, by, fit, **FIT_SCENES["fitted_in_range"][2])
    assert ndet == 1 and F(kw["max_range"]) < zx[0] <= F(5.25)


def test_many_keeps_the_first_64_by_start_index():
    bx, by, kw, fit, _ = FIT_SCENES["many"]
    zx, zy, ndet, stats = DF.detect_fit(bx, by, fit, **kw)
    cx, cy, _, _ = D.detect(bx, by, **kw)
    assert ndet == 64 and stats.tolist() == [70, 70, 64, 0]
    # each behind its centroid (the first 64 centroids, in their order) by at most the radius
    r, rc = np.hypot(zx.astype(np.float64), zy), np.hypot(cx.astype(np.float64), cy)
    assert np.all(r > rc) and np.all(r - rc <= 0.1 + 1e-5) and np.all(np.diff(zx) > 0)


def test_nan_and_inf_points():
    for name in ("nan_point", "inf_point", "minus_inf_point"):
        bx, by, kw, fit, _ = FIT_SCENES[name]
        zx, zy, ndet, stats = DF.detect_fit(bx, by, fit, **kw)
        assert ndet == 4 and np.isfinite(zx).all() and np.isfinite(zy).all(), name


def test_fit_validity():
    assert DF.fit_ok(DF.FIT_DEFAULT) and DF.fit_ok((1e-30, 0.0)) and DF.fit_ok((3e38, 3e38))
    for bad in ((0.0, 0.0), (-0.1, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.1, -1e-3), (0.1, float("nan")), (0.1, float("inf")),
                (1e-50, 0.0), (1e39, 0.0)):                                  # (tested on the float32 values: 1e-50 is 0, 1e39 inf)
        assert not DF.fit_ok(bad), bad


def test_arcs_of_64_points():
    """max_points = 64 with a segment of 64 points: fitted; 65 points: no segment of a legal size."""
    for lead, roll in ((3, 0), (30, 0), (3, -40)):
        bx, by, kw = FS.arc_scene(lead, roll=roll)
        zx, zy, ndet, stats = DF.detect_fit(bx, by, (0.1, 0.0), **kw)
        assert ndet == 1 and stats[3] == 0 and np.hypot(zx[0] - 2.0, zy[0] - 0.3) < 1e-3, (lead, roll)
        assert DF.detect_fit(bx, by, (0.1, 0.0), **dict(kw, wrap=0))[2] == (1 if roll == 0 else 0)
    bx, by, kw = FS.arc_scene(3, m=65)
    assert DF.detect_fit(bx, by, (0.1, 0.0), **kw)[2] == 0


@pytest.mark.parametrize("dist, bearing, m, half", [(5.0, 0.3, 7, 60.0), (2.0, -2.0, 4, 45.0), (10.0, 1.2, 3, 30.0), (20.0, 2.9, 16, 80.0),
                                                    (3.0, 0.0, 5, 70.0)])
def test_points_on_a_circle_give_its_centre(dist, bearing, m, half):
    """The derivation: p_i on the circle (C, rho), symmetric about the line of sight through C.  In exact arithmetic the fitted
    point IS C.  In float32 the distance is bounded from the magnitudes alone (u = 2^-24, R = |C| + rho bounds every coordinate):
      the points as float32:          each coordinate off by at most u R;
      the centroid:                   m - 1 additions and a division on numbers <= m R: off by at most eta_c = (m + 1) u R
                                      (with the points' own error);
      du, dv:                         off by eta = eta_c + 2 u R (the point's error, the subtraction's rounding);
      s2 (a mean of squares of |d| <= 2 rho):  2 |d| eta + the roundings of m + 3 operations on numbers <= 4 rho^2:
                                      ds2 = 4 rho eta + 4 (m + 3) u rho^2;
      t = rho2 - s2:                  dt = ds2 + 3 u rho^2 (rho2 rounded twice, the subtraction);
      d = sqrt(t):                    dd = dt / (2 delta) + u delta with delta the true distance centroid -> centre (sqrt's
                                      derivative at t = delta^2; delta, about rho sin(half) / half in radians, is > 0.6 rho here);
      the unit vector:                turned by at most eta_c / |c|, which moves the fitted point by delta eta_c / |c|, + 3 u delta;
      zx, zy:                         the sum's rounding, u R each.
    So |z - C| <= sqrt(2) (eta_c + dd + delta eta_c / |c| + 3 u delta + u R)."""
    rho = 0.1
    C = dist * np.array([np.cos(bearing), np.sin(bearing)])
    back = bearing + np.pi
    phi = back + np.deg2rad(np.linspace(-half, half, m))
    pts = np.stack([C[0] + rho * np.cos(phi), C[1] + rho * np.sin(phi)], 1)
    c = pts.mean(axis=0)
    delta = float(np.hypot(*(C - c)))
    assert abs(delta - np.sqrt(rho * rho - np.mean(np.sum((pts - c) ** 2, axis=1)))) < 1e-12       # the identity, in float64
    assert abs(c[0] * C[1] - c[1] * C[0]) < 1e-12 * dist * dist                                              # ... and the line of sight
    far = [(100.0, 50.0), (110.0, 50.0)]
    bx, by = FS._scan(far[:1] + pts.tolist() + far[1:])
    zx, zy, ndet, stats = DF.detect_fit(bx, by, (rho, 0.0), max_range=1000.0, min_points=3, max_points=64)
    assert ndet == 1 and stats.tolist() == [3, 1, 1, 0]
    R = dist + rho
    eta_c = (m + 1) * U * R
    eta = eta_c + 2 * U * R
    dt = 4 * rho * eta + 4 * (m + 3) * U * rho * rho + 3 * U * rho * rho
    dd = dt / (2 * delta) + U * delta
    bound = np.sqrt(2) * (eta_c + dd + delta * eta_c / np.hypot(*c) + 3 * U * delta + U * R)
    err = float(np.hypot(float(zx[0]) - C[0], float(zy[0]) - C[1]))
    print(f"dist {dist} m={m}: |z - C| = {err:.3e}, bound {bound:.3e}, centroid {delta:.4f} m in front")
    assert delta > 0.6 * rho and bound < 1e-4 * dist
    assert err <= bound
