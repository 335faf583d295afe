"""The edges of the pair-reseed specification (tests/_reseed_pair_spec.py), on the CPU: the accuracy of det_atan2, the draws, the
geometry of a proposal against a truth pose, the inclusive distance bounds on integers, and the counts."""
import functools

import numpy as np
import pytest

import _assoc_spec as A
import _reseed_pair_spec as RP
import _reseed_spec as R
import oracle

F = np.float32
U = 2.0**-24
SEED = 0x1234_5678_9ABC_DEF0
# the largest |det_atan2 - arctan2| measured by test_det_atan2_accuracy's own sweep (printed there; profiles/reseed_pairs.md), in
# [-pi, pi] and, behind the + 2 pi of a negative angle, in [0, 2 pi); the bounds are twice that, for inputs the sweep did not visit
ATAN2_MEASURED, ATAN2_WRAPPED_MEASURED = 2.54e-7, 5.08e-7
ATAN2_BOUND, ATAN2_WRAPPED_BOUND = 2 * ATAN2_MEASURED, 2 * ATAN2_WRAPPED_MEASURED
SINCOS_BOUND = 2.5e-7   # DESIGN.md "deterministic math": det_sincos on |x| <= 20, absolute


def atan2_sweep():
    """-> (y, x) float32: 4096 directions all round the circle at seven magnitudes from 1e-3 to 1e3 with the two components scaled
    apart as well; the four axes and the four diagonals; ratios min/max one to four ulps either side of tan(pi/8) (the reduction's
    boundary) and of 1 (the swap's) in all eight octants; and 65 536 random pairs whose magnitudes spread over the six decades."""
    rng = np.random.default_rng(17)
    ang = np.linspace(-np.pi, np.pi, 4096, endpoint=False) + 1e-4
    ys, xs = [], []
    for mag in (1e-3, 1e-2, 1e-1, 1.0, 1e1, 1e2, 1e3):
        ys.append(mag * np.sin(ang))
        xs.append(mag * np.cos(ang))
    for v in (1e-3, 1.0, 1e3):
        ys += [np.array([0.0, v, 0.0, -v, v, v, -v, -v])]
        xs += [np.array([v, 0.0, -v, 0.0, v, -v, v, -v])]
    for centre in (float(RP.TAN_PI_8), 1.0):
        big = F(3.0)
        small = F(centre) * big
        near = [small]
        for _ in range(4):
            near = [np.nextafter(near[0], F(0))] + near + [np.nextafter(near[-1], F(10))]
        near = np.array(near, F)
        for sy in (1, -1):
            for sx in (1, -1):
                ys += [sy * near, sy * np.full_like(near, big)]
                xs += [sx * np.full_like(near, big), sx * near]
    m = 10.0 ** rng.uniform(-3, 3, (2, 65536)) * rng.choice([-1.0, 1.0], (2, 65536))
    ys.append(m[0])
    xs.append(m[1])
    return np.concatenate(ys).astype(F), np.concatenate(xs).astype(F)


def atan2_error(y, x):
    """-> (largest |det_atan2 - arctan2| in [-pi, pi], the same behind the wrap into [0, 2 pi)) against float64 on the same inputs."""
    got = RP.det_atan2(y, x)
    want = np.arctan2(y.astype(np.float64), x.astype(np.float64))
    wrapped = np.where(got < 0, got + R.TWO_PI, got).astype(F)
    want_w = np.where(want < 0, want + 2 * np.pi, want)
    d = np.abs(wrapped.astype(np.float64) - want_w)
    d = np.minimum(d, 2 * np.pi - d)   # (-0.0...1 wraps to 2 pi as rounded: the same direction)
    return float(np.abs(got.astype(np.float64) - want).max()), float(d.max())


def test_det_atan2_accuracy():
    y, x = atan2_sweep()
    plain, wrapped = atan2_error(y, x)
    print(f"det_atan2 over {len(y)} inputs: largest error {plain:.3e} rad in [-pi, pi], {wrapped:.3e} rad behind the wrap to [0, 2 pi)")
    assert plain <= ATAN2_BOUND and wrapped <= ATAN2_WRAPPED_BOUND
    assert plain >= 0.5 * ATAN2_MEASURED and wrapped >= 0.5 * ATAN2_WRAPPED_MEASURED, "the recorded figures are not this sweep's"
    # the octants exactly: axes and diagonals up to the rounding of the constants, and the sign symmetries bit for bit
    ax = RP.det_atan2(F([0, 1, 0, -1, 1, 1, -1, -1]), F([1, 0, -1, 0, 1, -1, 1, -1]))
    assert np.allclose(ax, [0, np.pi / 2, np.pi, -np.pi / 2, np.pi / 4, 3 * np.pi / 4, -np.pi / 4, -3 * np.pi / 4], atol=2e-7, rtol=0)
    nz = y != 0
    assert np.array_equal(RP.det_atan2(-y[nz], x[nz]), -RP.det_atan2(y[nz], x[nz]))
    with pytest.raises(AssertionError):
        RP.det_atan2(F([0.0]), F([0.0]))


def test_draws_pick_two_different_detections_uniformly(orc):
    n = 1 << 16
    for K in (2, 3, 5, 64):
        r0, j1, k1, k2, rb0 = RP.draws(n, 2**32 + 5, SEED, 3, 12, K)
        assert np.all(k2 != k1) and k1.min() == 0 and k1.max() == K - 1 and k2.min() == 0 and k2.max() == K - 1
        if K <= 5:   # for every k1, k2 is uniform over the K - 1 others: each count within 5 sigma of its binomial
            for a in range(K):
                tot = int((k1 == a).sum())
                for b in range(K):
                    got = int(((k1 == a) & (k2 == b)).sum())
                    p = 0.0 if a == b else 1.0 / (K - 1)
                    assert abs(got - tot * p) <= 5 * np.sqrt(tot * p * (1 - p)) + 1e-9, (K, a, b, got, tot)
    # the single-detection spec draws the same first word, landmark and first detection
    s0, sj, sk, _ = R.draws(n, 2**32 + 5, SEED, 3, 12, 5)
    r0, j1, k1, k2, rb0 = RP.draws(n, 2**32 + 5, SEED, 3, 12, 5)
    assert np.array_equal(s0, r0) and np.array_equal(sj, j1) and np.array_equal(sk, k1) and not np.array_equal(rb0, r0)


def test_the_chosen_slots_are_the_single_reseeds(orc):
    n = 8192
    rng = np.random.default_rng(4)
    x, y, th = (rng.standard_normal(n).astype(F) for _ in range(3))
    M = truth_map()
    zx, zy = truth_detections(M, TRUTH)
    for fraction in (1.0 / 16, 0.5, 1.0):
        single = R.reseed(M, x, y, th, None, zx, zy, 7, SEED, 2, fraction)[3]
        pair = RP.reseed_pairs(M, x, y, th, None, zx, zy, 7, SEED, 2, fraction, TOL, MIN_SEP)[3]
        assert np.array_equal(single != 0, pair != 0) and (pair != 0).sum() > 0


TRUTH = (3.25, -1.5, 0.7)
TOL, MIN_SEP = 0.05, 1.0


@functools.lru_cache(maxsize=None)
def _truth_map():
    """12 landmarks whose 66 pairwise distances all differ by more than 2 TOL from one another (asserted)."""
    rng = np.random.default_rng(0)
    for _ in range(10000):
        p = rng.uniform(-40, 40, (12, 2)).astype(F)
        d = np.sort(np.hypot(*(p[:, None] - p[None]).transpose(2, 0, 1).astype(np.float64))[np.triu_indices(12, 1)])
        if np.diff(d).min() > 2 * TOL + 1e-3 and d.min() > MIN_SEP + 2 * TOL:
            break
    else:
        raise AssertionError("no such map")
    M = np.zeros((5, 12), F)
    M[0], M[1], M[2], M[4] = p[:, 0], p[:, 1], 0.05, 0.05
    return M


def truth_map():
    return _truth_map().copy()


def truth_detections(M, pose, which=range(9)):
    """The landmarks `which` seen exactly from pose: z = H(theta) (m - p), H = [[c, -s], [s, c]], in double, rounded once."""
    px, py, t = pose
    dx, dy = M[0][list(which)].astype(np.float64) - px, M[1][list(which)].astype(np.float64) - py
    c, s = np.cos(t), np.sin(t)
    return (c * dx - s * dy).astype(F), (s * dx + c * dy).astype(F)


def heading_bound(a_len, z1, z2):
    """How far the proposal's heading can lie from the angle of a less the angle of b, from the operations used:
    each z is a rounded double (u |z|_1 over its two components); a = z_k2 - z_k1 adds u |a|_1; b = m_j2 - m_j1 is u |b|_1 off; a
    vector that is delta off turns by at most delta / its length.  cr and dt are two products and one sum each: by Cauchy-Schwarz
    |bx ay| + |by ax| <= |a| |b|, so each is within 2u |a| |b| (1 + u), and atan2 turns by at most (|d cr| + |d dt|) / (|a| |b|) —
    4u, taken as 6u for the second order.  Then det_atan2 and the wrap into [0, 2 pi): ATAN2_WRAPPED_BOUND."""
    da = U * (z1 + z2) + U * (np.sqrt(2.0) * a_len)
    return ATAN2_WRAPPED_BOUND + da / a_len + U * np.sqrt(2.0) + 6 * U


def test_geometry_against_a_truth_pose(orc):
    n = 4096
    M = truth_map()
    zx, zy = truth_detections(M, TRUTH)
    K = len(zx)
    assert K == 9
    x = y = th = np.zeros(n, F)
    xo, yo, to, flag, counts = RP.reseed_pairs(M, x, y, th, None, zx, zy, 0, SEED, 5, 1.0, TOL, MIN_SEP)
    r0, j1, k1, k2, rb0 = RP.draws(n, 0, SEED, 5, 12, K)
    assert counts[1] == 0 and counts[2] == 0 and counts.sum() == n
    right = (flag == 1) & (j1 == k1)          # detection k was made from landmark k
    assert right.sum() >= 1
    print(f"replaced {counts[0]} of {n}; {int(right.sum())} with the first detection on its own landmark; no partner {counts[3]}")
    assert np.all(flag[j1 == k1] == 1)        # the true partner is always there
    z1 = np.abs(zx[k1]).astype(np.float64) + np.abs(zy[k1])
    z2 = np.abs(zx[k2]).astype(np.float64) + np.abs(zy[k2])
    a_len = np.hypot(zx[k2].astype(np.float64) - zx[k1], zy[k2].astype(np.float64) - zy[k1])
    hb = heading_bound(a_len, z1, z2)
    # at the truth: the heading within hb; the position within |z_k1| (hb + the sine's and cosine's error) — the lever of the
    # heading — plus z's own rounding (u |z|_1), the three roundings of t (3u |z|_1) and of x' = mx - t (u (|m| + |z|_1))
    dth = np.abs(to.astype(np.float64) - TRUTH[2])
    dth = np.minimum(dth, 2 * np.pi - dth)
    lever = np.hypot(zx[k1].astype(np.float64), zy[k1])
    pos_bound = lever * (hb + 2 * SINCOS_BOUND) + 4 * U * z1 + U * (np.abs(M[:2, j1]).max(axis=0) + z1)
    err = np.hypot(xo.astype(np.float64) - TRUTH[0], yo.astype(np.float64) - TRUTH[1])
    print(f"at the truth: largest heading error {dth[right].max():.3e} rad (bound {hb[right].min():.3e} or more), "
          f"largest position error {err[right].max():.3e} m (bound {pos_bound[right].min():.3e} or more)")
    assert np.all(dth[right] <= hb[right]) and np.all(err[right] <= pos_bound[right])
    # every replaced proposal, right or wrong: k1 is observed at m_j1 within test_reseed_spec_cpu.py's bound, and k2 at some
    # landmark other than j1 within tol (the lengths of a and b) plus the heading bound times |a| (the directions)
    rep = flag == 1
    s, c = oracle.det_sincos(to)
    w1 = A.observed_point(zx[k1], zy[k1], s, c, xo, yo)
    T = z1 * (1 + 2.0**-20)
    for w, m in zip(w1, (M[0][j1].astype(np.float64), M[1][j1].astype(np.float64))):
        bound = U * (np.abs(m) + T) + U * (np.abs(m) + U * (np.abs(m) + T))
        assert np.all(np.abs(w.astype(np.float64) - m)[rep] <= bound[rep])
    cs, sn = np.cos(to.astype(np.float64)), np.sin(to.astype(np.float64))
    w2x = xo + cs * zx[k2] + sn * zy[k2]
    w2y = yo + cs * zy[k2] - sn * zx[k2]
    dist = np.hypot(w2x[:, None] - M[0][None].astype(np.float64), w2y[:, None] - M[1][None].astype(np.float64))
    dist[np.arange(n), j1] = np.inf
    slack = dist.min(axis=1) - (TOL + hb * a_len)
    print(f"second detection: largest distance from a landmark less its bound {slack[rep].max():.3e} m")
    assert np.all(slack[rep] <= 0)


def test_both_distance_bounds_are_inclusive_on_integers(orc):
    """tol = 0, a = +-(3, 4): dz2 = 25 = lo2 = hi2 exactly.  Landmarks 0 and 5 stand on one spot; from there (3, 4), (5, 0) and
    (4, 3) are partners — dm2 = 25 on both bounds at once —, (6, 0) is not, and the twin on the same spot is not (dm2 = 0)."""
    m = np.array([10.0, 20.0])
    off = np.array([(0, 0), (3, 4), (5, 0), (4, 3), (6, 0), (0, 0)], np.float64)
    M = np.zeros((5, 6), F)
    M[0], M[1], M[2], M[4] = m[0] + off[:, 0], m[1] + off[:, 1], 0.05, 0.05
    zx, zy = F([1.0, 4.0]), F([2.0, 6.0])
    for j in (0, 5):
        assert RP.partners(M, j, F(25.0), F(25.0)).tolist() == [False, True, True, True, False, False]
    n = 2048
    x = y = th = np.zeros(n, F)
    xo, yo, to, flag, counts = RP.reseed_pairs(M, x, y, th, None, zx, zy, 0, SEED, 1, 1.0, 0.0, 1.0)
    r0, j1, k1, k2, rb0 = RP.draws(n, 0, SEED, 1, 6, 2)
    here = np.isin(j1, (0, 5))
    assert here.sum() > 100 and np.all(flag[here] == 1) and counts.sum() == n
    # which partner a proposal took: the landmark its second detection is observed at
    cs, sn = np.cos(to.astype(np.float64)), np.sin(to.astype(np.float64))
    w2 = np.stack([xo + cs * zx[k2] + sn * zy[k2], yo + cs * zy[k2] - sn * zx[k2]], axis=1)
    took = np.argmin(np.hypot(*(w2[:, None] - (m + off)[None]).transpose(2, 0, 1)), axis=1)
    assert set(took[here].tolist()) == {1, 2, 3}
    assert np.all(np.hypot(*(w2[here] - (m + off)[took[here]]).T) < 1e-4)
    # (6, 0) has one partner only — the landmark at (3, 4) is 5 away from it — and it is always taken
    assert np.all(flag[j1 == 4] == 1) and set(took[j1 == 4].tolist()) == {1}


def test_the_four_counts_and_the_unchosen_add_up(orc):
    n = 1 << 14
    rng = np.random.default_rng(9)
    x, y, th = (rng.standard_normal(n).astype(F) for _ in range(3))
    anc = rng.integers(0, n, n).astype(np.int32)
    M = truth_map()
    M[2, ::4] = -1.0
    zx, zy = truth_detections(M, TRUTH, which=range(1, 9))
    zx, zy = np.append(zx, zx[0] + F(0.25)), np.append(zy, zy[0])      # a pair closer than min_sep
    zx, zy = np.append(zx, F(np.nan)), np.append(zy, F(0.0))            # and a detection that is not a number: too close
    xo, yo, to, flag, counts = RP.reseed_pairs(M, x, y, th, anc, zx, zy, 0, SEED, 8, 0.5, TOL, MIN_SEP)
    unchosen = int((flag == 0).sum())
    print("counts", counts.tolist(), "unchosen", unchosen)
    assert np.all(counts > 0) and counts.sum() + unchosen == n and abs(unchosen - n / 2) < 5 * np.sqrt(n / 4)
    assert [int((flag == v).sum()) for v in (1, 2, 3, 4)] == counts.tolist()
    keep = flag != 1
    assert np.array_equal(xo[keep], x[anc][keep]) and np.array_equal(yo[keep], y[anc][keep]) and np.array_equal(to[keep], th[anc][keep])
    assert np.all(np.isfinite(xo[~keep])) and np.all((to[~keep] >= 0) & (to[~keep] <= F(6.2831855)))
    r0, j1, k1, k2, rb0 = RP.draws(n, 0, SEED, 8, 12, len(zx))
    assert np.all(flag[(flag != 0) & ((k1 == 9) | (k2 == 9))] == 3)     # the NaN
    # K < 2 writes nothing; the parameters are checked
    assert RP.reseed_pairs(M, x, y, th, None, zx[:1], zy[:1], 0, SEED, 8, 0.5, TOL, MIN_SEP)[0] is None
    for tol, sep in ((-0.1, 1.0), (0.5, 0.5), (0.0, float("inf")), (float("nan"), 1.0), (0.0, float("nan"))):
        with pytest.raises(ValueError):
            RP.reseed_pairs(M, x, y, th, None, zx, zy, 0, SEED, 8, 0.5, tol, sep)
