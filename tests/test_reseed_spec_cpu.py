"""The edges of the reseed specification (tests/_reseed_spec.py), on the CPU: the threshold at both ends of the fraction, the
geometry of a proposal, empty map slots, the high word of the particle id, the replaced share, and the vectorised Philox against
the oracle's."""
import numpy as np
import pytest

import _assoc_spec as A
import _reseed_spec as R
import oracle

F = np.float32
SEED = 0x1234_5678_9ABC_DEF0


def cloud(n, seed=3, scale=10.0):
    rng = np.random.default_rng(seed)
    return tuple((scale * rng.standard_normal(n)).astype(F) for _ in range(3))


def one_map(L, empty=()):
    rng = np.random.default_rng(11)
    M = np.zeros((5, L), F)
    M[0], M[1] = rng.uniform(-50, 50, (2, L)).astype(F)
    M[2] = M[4] = 0.05
    M[2, list(empty)] = -1.0
    return M


def test_vectorised_philox_is_the_oracles(orc):
    rng = np.random.default_rng(5)
    ctr = rng.integers(0, 2**32, (64, 4), dtype=np.uint64).astype(np.uint32)
    ctr[0], ctr[1] = 0, 0xffffffff
    for key in ((0, 0), (0xffffffff, 0xffffffff), (SEED & 0xffffffff, SEED >> 32)):
        got = R.philox(ctr[:, 0], ctr[:, 1], ctr[:, 2], ctr[:, 3], *key)
        for i in range(len(ctr)):
            assert [int(g[i]) for g in got] == [int(v) for v in oracle.philox(ctr[i], key)]


def test_threshold_at_both_ends(orc):
    assert R.threshold(1.0) == 2**32 and R.threshold(2.0**-32) == 1 and R.threshold(0.5) == 2**31
    for bad in (0.0, -0.5, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            R.threshold(bad)
    n = 4096
    x, y, th = cloud(n)
    M, zx, zy = one_map(7), np.array([1.0, -2.0], F), np.array([0.5, 3.0], F)
    *_, flag, counts = R.reseed(M, x, y, th, None, zx, zy, 0, SEED, 4, 1.0)
    assert np.all(flag == 1) and tuple(counts) == (n, 0)          # fraction 1: every slot, whatever its first word
    r0 = R.draws(n, 0, SEED, 4, 7, 2)[0]
    xo, yo, to, flag, counts = R.reseed(M, x, y, th, None, zx, zy, 0, SEED, 4, 2.0**-32)
    assert np.array_equal(flag != 0, r0 == 0) and counts.sum() == int((r0 == 0).sum())   # threshold 1: only a first word of 0
    keep = flag == 0
    assert np.array_equal(xo[keep], x[keep]) and np.array_equal(yo[keep], y[keep]) and np.array_equal(to[keep], th[keep])


@pytest.mark.parametrize("m, z", [((3.0, -4.0), (2.0, 1.5)), ((1000.0, -1000.0), (25.0, -7.0)), ((0.0, 0.0), (0.3, 0.0)),
                                  ((-512.25, 77.125), (-60.0, 60.0))])
def test_every_proposal_observes_the_landmark_where_the_map_has_it(orc, m, z):
    """K = 1, L = 1.  x' = fl(mx - t) and the update's w_x = fl(x' + t) with the SAME t (the same s, c, z and operations, bit for
    bit), so of the roundings only these two per coordinate — four in all — do not cancel.  With u = 2^-24:
        |x' - (mx - t)| <= u |mx - t| <= u (|mx| + |t|)
        |w_x - (x' + t)| <= u |x' + t| <= u (|mx| + u (|mx| + |t|))
    and |t| <= (|zx| + |zy|) (1 + 2^-20): two products by |s|, |c| <= 1 + 2^-22 (the polynomials' error) and one sum."""
    n = 4096
    x, y, th = cloud(n)
    M = np.zeros((5, 1), F)
    M[:, 0] = (m[0], m[1], 0.05, 0.0, 0.05)
    zx, zy = np.array([z[0]], F), np.array([z[1]], F)
    xo, yo, to, flag, counts = R.reseed(M, x, y, th, None, zx, zy, 0, SEED, 9, 1.0)
    assert tuple(counts) == (n, 0) and np.all((to >= 0) & (to < F(6.2831855)))
    s, c = oracle.det_sincos(to)
    wx, wy = A.observed_point(zx[0], zy[0], s, c, xo, yo)
    u, T = 2.0**-24, (abs(float(zx[0])) + abs(float(zy[0]))) * (1 + 2.0**-20)
    for w, mv in ((wx, float(M[0, 0])), (wy, float(M[1, 0]))):
        bound = u * (abs(mv) + T) + u * (abs(mv) + u * (abs(mv) + T))
        err = np.abs(w.astype(np.float64) - mv).max()
        print(f"m = {mv}: largest error {err:.3e}, bound {bound:.3e}")
        assert err <= bound
    # the proposals lie on the circle of radius |z| around the landmark, all round it
    rad = np.hypot(xo.astype(np.float64) - m[0], yo.astype(np.float64) - m[1])
    assert np.allclose(rad, np.hypot(*z), rtol=1e-5, atol=1e-4) and len(np.unique(to)) > n // 2


def test_an_empty_map_slot_leaves_the_resampled_pose_and_is_counted(orc):
    n, L = 8192, 5
    x, y, th = cloud(n)
    anc = np.random.default_rng(2).integers(0, n, n).astype(np.int32)
    M = one_map(L, empty=(1, 3))
    zx, zy = np.array([1.0, -2.0, 0.25], F), np.array([0.5, 3.0, -4.0], F)
    xo, yo, to, flag, counts = R.reseed(M, x, y, th, anc, zx, zy, 0, SEED, 2, 0.5)
    r0, j, k, theta = R.draws(n, 0, SEED, 2, L, 3)
    chosen = r0 < 2**31
    empty = chosen & np.isin(j, (1, 3))
    assert empty.sum() > 100 and np.array_equal(flag == 2, empty) and np.array_equal(flag == 1, chosen & ~empty)
    assert tuple(counts) == (int((flag == 1).sum()), int(empty.sum()))
    keep = flag != 1
    assert np.array_equal(xo[keep], x[anc][keep]) and np.array_equal(yo[keep], y[anc][keep]) and np.array_equal(to[keep], th[anc][keep])
    assert np.array_equal(to[~keep], theta[~keep]) and j.max() == L - 1 and j.min() == 0 and set(np.unique(k)) == {0, 1, 2}


def test_the_high_word_of_the_particle_id_changes_the_draws(orc):
    n = 512
    low, high = R.draws(n, 7, SEED, 1, 50, 20), R.draws(n, 2**32 + 7, SEED, 1, 50, 20)
    assert not np.array_equal(low[0], high[0]) and not np.array_equal(low[3], high[3])
    again = R.draws(n, 2**32 + 7, SEED, 1, 50, 20)
    assert all(np.array_equal(a, b) for a, b in zip(high, again))
    assert not np.array_equal(high[0], R.draws(n, 2**32 + 7, SEED, 2, 50, 20)[0])          # the frame word
    assert not np.array_equal(high[0], R.draws(n, 2**32 + 7, SEED ^ (1 << 40), 1, 50, 20)[0])   # the high word of the seed


def test_the_replaced_share_is_binomial(orc):
    n = 1 << 20
    x = y = th = np.zeros(n, F)
    M, zx, zy = one_map(3), np.array([1.0], F), np.array([0.5], F)
    for fraction in (float(F(0.3)), 1.0 / 16):
        p = R.threshold(fraction) / 2.0**32
        counts = R.reseed(M, x, y, th, None, zx, zy, 0, SEED, 6, fraction)[4]
        sigma = np.sqrt(n * p * (1 - p))
        print(f"fraction {fraction}: replaced {counts[0]} of {n}, expected {n * p:.0f} +- {sigma:.0f}")
        assert counts[1] == 0 and abs(counts[0] - n * p) <= 5 * sigma
