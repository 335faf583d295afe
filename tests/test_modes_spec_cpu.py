"""The definition of slam_pf_modes (tests/_modes_spec.py) against float64 and against itself: what the GPU tests hold the device
to bit for bit is first shown to be the right thing.  Needs no GPU."""
import math

import numpy as np
import pytest

import _estimate_spec as E
import _modes_spec as M
import _spread_spec as S

CELL, H, MM = 0.5, 8, 4
EPS = 2.0 ** -24     # half an ulp of binary32, relative


def xy_bound(cell, max_abs):
    """|mode coordinate - float64 weighted mean of its members' coordinate|, from the roundings of the definition:
      inv = fl(1 / cell) and u = fl(x * inv): two relative roundings of 2^-24, so |u * cell - x| <= (2 eps + eps^2) |x| per particle;
      u - floor(u) is exact, except that it rounds to 1.0f for u in (-2^-25, 0): 2^-24 cells at most;
      F = trunc(frac * 2^20) loses less than 2^-20 cells per particle, and the truncating division of the sums less than 2^-20 more;
      the final product is formed in binary64 and rounded once to binary32: one more relative 2^-24 (the binary64 steps are
      2^-53 each, far below).
    Three relative roundings at 2^-24; a fourth covers the second-order terms and the binary64 steps."""
    return cell * (2.0 ** -19 + 2.0 ** -24) + 4.0 * EPS * max_abs


def theta_bound(r_min, max_abs_theta):
    """S and C lose less than 2^-20 each to the cast and no more than 2^-22 to the polynomial (Cephes' single-precision sets: below
    2 ulp of a value <= 1); an error (ds, dc) of the mean vector of length R turns it by at most hypot(ds, dc) / R.  theta - ref is
    one binary32 subtraction per particle and the result is rounded once: 2^-24 relative each; a third covers binary64's atan2."""
    return math.hypot(2.0 ** -20 + 2.0 ** -22, 2.0 ** -20 + 2.0 ** -22) / r_min + 3.0 * EPS * max_abs_theta


def members_of(mode, x, y, th, cell, hbins, ref=0.0):
    ix, iy, b, *_ = M.particle_terms(x, y, th, None, ref, cell, hbins)
    c = mode.cell
    hd = np.minimum(np.abs(b - c[2]), hbins - np.abs(b - c[2]))
    return (np.abs(ix - c[0]) <= 1) & (np.abs(iy - c[1]) <= 1) & (hd <= 1)


@pytest.mark.parametrize("n", [257, 4097])
def test_two_clusters_are_two_modes_where_the_mean_is_nowhere(n):
    x, y, th = S.spread_population("two_clusters", n)
    ref = 0.5
    r = M.modes_spec(x, y, th, None, ref, CELL, H, MM)
    assert len(r.modes) == 2 and r.wtotal == n
    for m in r.modes:
        assert abs(float(m.mass) - 0.5) <= 1.0 / n
        sel = members_of(m, x, y, th, CELL, H)
        assert int(sel.sum()) == m.weight
        x64, y64, t64 = (a[sel].astype(np.float64) for a in (x, y, th))
        assert abs(float(m.pose[0]) - x64.mean()) <= xy_bound(CELL, np.abs(x64).max()), (m, x64.mean())
        assert abs(float(m.pose[1]) - y64.mean()) <= xy_bound(CELL, np.abs(y64).max()), (m, y64.mean())
        d = t64 - float(np.float32(ref))
        ms, mc = np.sin(d).mean(), np.cos(d).mean()
        want = float(np.float32(ref)) + math.atan2(ms, mc)
        assert abs(float(m.pose[2]) - want) <= theta_bound(math.hypot(ms, mc), 4.0), (m, want)
    assert {m.cell[2] for m in r.modes} == {0, 4}
    pose, _ = E.mean_spec(x, y, th, None, ref, n)
    assert np.hypot(x.astype(np.float64) - float(pose[0]), y.astype(np.float64) - float(pose[1])).min() > 3.0


def test_permutation_invariance():
    n = 4097
    rng = np.random.default_rng(5)
    logw = rng.normal(-3.0, 1.5, n).astype(np.float32)
    w16, _ = M.weights16(logw)
    for name, pop in (("two_clusters", S.spread_population("two_clusters", n)), ("scatter", M.modes_population("scatter", n))):
        p = rng.permutation(n)
        for w in (None, w16):
            a = M.modes_spec(*pop, None, 0.3, CELL, H, MM, w)
            b = M.modes_spec(*(v[p] for v in pop), None, 0.3, CELL, H, MM, None if w is None else [w[i] for i in p])
            assert M.same(a, b), name
        # a gather is a permutation as well
        assert M.same(M.modes_spec(*pop, None, 0.3, CELL, H, MM), M.modes_spec(*(v[p] for v in pop), np.argsort(p), 0.3, CELL, H, MM))


def test_floor_not_the_cast():
    x, y, th = M.modes_population("straddle_zero", 1025, CELL)
    r = M.modes_spec(x, y, th, None, 1.0, CELL, H, MM)
    cells = M.cell_table(x, y, th, None, 1.0, CELL, H)
    assert {k[0] for k in cells} == {-1, 0} and {k[1] for k in cells} == {-1, 0}
    assert len(r.modes) == 1 and r.modes[0].ncells == len(cells) and r.modes[0].weight == 1025
    assert abs(float(r.modes[0].pose[0]) - x.astype(np.float64).mean()) <= xy_bound(CELL, float(np.abs(x).max()))
    wrong = M.cell_table(x, y, th, None, 1.0, CELL, H, floor=np.trunc)
    assert {k[0] for k in wrong} == {0} and not M.same(r, M.modes_spec(x, y, th, None, 1.0, CELL, H, MM, floor=np.trunc))


def test_headings_across_zero_are_one_mode():
    n = 1024
    x, y, th = M.modes_population("heading_wrap", n, CELL)
    for ref in (0.0, 3.0):
        r = M.modes_spec(x, y, th, None, ref, CELL, H, MM)
        cells = M.cell_table(x, y, th, None, ref, CELL, H)
        assert {k[2] for k in cells} == {0, H - 1}
        assert len(r.modes) == 1 and r.modes[0].weight == n
        *_, want, rlen = E.f64_means(x, y, th, ref)
        got = float(r.modes[0].pose[2])
        assert abs(math.remainder(got - want, 2.0 * math.pi)) <= theta_bound(rlen, 8.0), (got, want)
        assert abs(math.remainder(got, 2.0 * math.pi)) < 0.01


def test_three_cells_apart_two_modes_two_cells_apart_one_centre():
    n = 512
    three = M.modes_spec(*M.two_blobs(n, 3, CELL), None, 1.0, CELL, H, MM)
    assert [m.cell for m in three.modes] == [(10, 7, 1), (13, 7, 1)] and [m.weight for m in three.modes] == [n // 2, n // 2]
    two = M.modes_spec(*M.two_blobs(n, 2, CELL), None, 1.0, CELL, H, MM)
    assert [m.cell for m in two.modes] == [(10, 7, 1)] and two.modes[0].weight == n // 2 and two.cells == 2
    assert two.modes[0].mass == np.float32(0.5)
    # ... and the heavier of the two is the one centre, whichever side it lies on
    heavy = M.modes_spec(*M.two_blobs(n, 2, CELL, weight_ratio=1), None, 1.0, CELL, H, MM,
                         w16=[1 if i % 2 == 0 else 3 for i in range(n)])
    assert [m.cell for m in heavy.modes] == [(12, 7, 1)] and heavy.modes[0].weight == 3 * n // 2


def test_equal_weights_smaller_key_first_and_max_modes_one():
    n = 512
    pop = M.two_blobs(n, 5, CELL)
    r = M.modes_spec(*pop, None, 1.0, CELL, H, MM)
    assert [m.cell for m in r.modes] == [(10, 7, 1), (15, 7, 1)] and r.modes[0].weight == r.modes[1].weight
    # negative cells compare as signed integers
    neg = (pop[0] - np.float32(20.0 * CELL), pop[1], pop[2])
    assert [m.cell[0] for m in M.modes_spec(*neg, None, 1.0, CELL, H, MM).modes] == [-10, -5]
    one = M.modes_spec(*pop, None, 1.0, CELL, H, 1)
    assert len(one.modes) == 1 and M.same(M.Result(r.modes[:1], r.cells, r.wtotal), one)


def test_weight_zero_makes_no_cell():
    n = 512
    x, y, th = M.two_blobs(n, 5, CELL)
    w = [0 if i % 2 else 7 for i in range(n)]          # the second cluster has no weight at all
    r = M.modes_spec(x, y, th, None, 1.0, CELL, H, MM, w16=w)
    assert r.cells == 1 and len(r.modes) == 1 and r.modes[0].weight == 7 * n // 2 and r.wtotal == 7 * n // 2
    assert r.modes[0].mass == np.float32(1.0)
    # no weight anywhere: the plain form
    assert M.same(M.modes_spec(x, y, th, None, 1.0, CELL, H, MM, w16=[0] * n), M.modes_spec(x, y, th, None, 1.0, CELL, H, MM))


def test_one_heading_bin():
    x, y, th = S.spread_population("two_clusters", 513)
    r = M.modes_spec(x, y, th, None, 0.5, CELL, 1, MM)
    assert len(r.modes) == 2 and all(m.cell[2] == 0 for m in r.modes)
    assert max(len(M.neighbours((0, 0, 0), 1)), 0) == 9 and len(M.neighbours((0, 0, 0), 8)) == 27 and len(M.neighbours((0, 0, 7), 4)) == 27


def test_capacity_and_domain_verdicts():
    th = np.zeros(M.MAX_CELLS + 1, np.float32)
    x = (np.arange(M.MAX_CELLS + 1) * CELL).astype(np.float32)
    y = np.zeros_like(x)
    with pytest.raises(M.TooManyCells):
        M.modes_spec(x, y, th, None, 0.0, CELL, H, MM)
    ok = M.modes_spec(x[:-1], y[:-1], th[:-1], None, 0.0, CELL, H, MM)
    assert ok.cells == M.MAX_CELLS and len(ok.modes) == MM
    small = [np.array(v, np.float32) for v in ([1.0, 2.0, 3.0], [0.0, 0.0, 0.0], [0.1, 0.2, 0.3])]
    inside = np.nextafter(np.float32(2.0 ** 20 * CELL), np.float32(0.0))
    for axis in (0, 1):
        for sign in (1.0, -1.0):
            bad = [a.copy() for a in small]
            bad[axis][1] = np.float32(sign * 2.0 ** 20 * CELL)      # u = +-2^20 exactly
            with pytest.raises(M.OutOfDomain):
                M.modes_spec(*bad, None, 0.0, CELL, H, MM)
            bad[axis][1] = np.float32(sign) * inside
            r = M.modes_spec(*bad, None, 0.0, CELL, H, MM)
            assert (2 ** 20 - 1 if sign > 0 else -2 ** 20) in {m.cell[axis] for m in r.modes}
    for axis in (0, 1, 2):
        bad = [a.copy() for a in small]
        bad[axis][2] = np.nan
        with pytest.raises(M.OutOfDomain):
            M.modes_spec(*bad, None, 0.0, CELL, H, MM)
    # the domain comes first: one particle outside among too many cells
    x[5] = np.float32(np.inf)
    with pytest.raises(M.OutOfDomain):
        M.modes_spec(x, y, th, None, 0.0, CELL, H, MM)
    assert not M.params_ok(0.0, H, MM) and not M.params_ok(np.inf, H, MM) and not M.params_ok(CELL, 2, MM)
    assert not M.params_ok(CELL, 65, MM) and not M.params_ok(CELL, H, 0) and not M.params_ok(CELL, H, 9) and M.params_ok(CELL, 1, 8)
