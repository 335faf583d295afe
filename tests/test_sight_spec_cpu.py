"""tests/_sight_spec.py by hand: the bin of a point on the axes, the diagonals and the edges of the rule; the sight table; and the
evidence stage with it — equal to tests/_evidence_spec.py when nothing hides anything, a hit on a hidden landmark, a landmark
nearer than the margin, and a landmark's own pole.  No GPU."""
import numpy as np
import pytest

import _evidence_spec as E
import _sight_spec as S

F = np.float32
TINY = float(np.float32(1e-45))   # the smallest subnormal
INF = float("inf")


def one_bin(x, y, bins):
    j, has = S.bin_of(np.array([x], F), np.array([y], F), bins)
    return int(j[0]) if has[0] else None


@pytest.mark.parametrize("bins", [32, 1024])
def test_axes_and_diagonals(bins):
    q = bins // 4
    for (x, y), p in (((1, 0), 0), ((0, 1), 1), ((-1, 0), 2), ((0, -1), 3), ((3, 3), 0.5), ((-2, 2), 1.5), ((-0.5, -0.5), 2.5), ((7, -7), 3.5)):
        assert one_bin(x, y, bins) == int(p * q), (x, y)
    # the bins are contiguous sectors in the order of the true angle
    a = np.linspace(-np.pi, np.pi, 20001)[1:]
    j, has = S.bin_of(np.cos(a).astype(F), np.sin(a).astype(F), bins)
    assert has.all()
    step = np.diff(np.concatenate([j[a >= 0], j[a < 0]]))   # from angle 0 once round
    assert set(step.tolist()) <= {0, 1} and j[a >= 0][0] == 0 and j[a < 0][-1] == bins - 1
    assert len(set(j.tolist())) == bins


def test_the_edges_of_the_rule():
    assert one_bin(1.0, -TINY, 32) == 0            # q = 1e-45, p = 4 - q rounds to 4: wraps to bin 0
    assert one_bin(1.0, -TINY, 1024) == 0
    assert one_bin(1.0, -1e-3, 1024) == 1023       # ... and a little further down it is the last bin
    assert one_bin(1.0, -0.0, 32) == 0             # -0.0 is not negative: the first quadrant
    assert one_bin(-0.0, 1.0, 32) == 8
    assert one_bin(-0.0, -1.0, 32) == 24           # x >= 0, y < 0: p = 4 - 1
    assert one_bin(-1.0, -0.0, 32) == 16           # x < 0, y >= 0: p = 2 - 0
    for x, y in ((0.0, 0.0), (-0.0, 0.0), (INF, 1.0), (1.0, -INF), (np.nan, 1.0), (1.0, np.nan), (3e38, 3e38)):
        assert one_bin(x, y, 32) is None, (x, y)
    assert one_bin(TINY, 0.0, 32) == 0 and one_bin(0.0, TINY, 32) == 8   # the smallest points there are have bins


def test_the_table():
    bx = np.array([2.0, 3.0, 0.0, 0.0, -1.0, INF, 1.0], F)
    by = np.array([0.1, 0.1, 0.0, 2.0, -1.0, 1.0, 0.0], F)
    T = S.table(bx, by, 32)
    assert T.dtype == np.float32 and T.shape == (32,)
    want = np.full(32, np.inf, F)
    want[0] = F(1.0)                               # (2, .1), (3, .1) and (1, 0) share bin 0: the minimum
    want[8] = F(4.0)
    want[20] = F(2.0)                              # (the origin and the inf point add nothing)
    assert np.array_equal(T, want)
    rng = np.random.default_rng(1)
    bx, by = (rng.standard_normal(500) * 5).astype(F), (rng.standard_normal(500) * 5).astype(F)
    T = S.table(bx, by, 128)
    assert np.isinf(S.table(bx[:3], by[:3], 1024)).sum() >= 1021
    for _ in range(5):
        p = rng.permutation(500)
        assert np.array_equal(S.table(bx[p], by[p], 128).view(np.uint32), T.view(np.uint32))
    assert np.all(T[np.isfinite(T)] > 0) and not np.isnan(T).any()
    assert np.array_equal(S.table(np.zeros(0, F), np.zeros(0, F), 64), np.full(64, np.inf, F))


# ------------------------------------------------------------------ the evidence stage
HIT, MISS, CMAX, RANGE = 2, 1, 8, 9.0
POSE = (0.5, -0.25, 0.7)


def to_world(zx, zy, pose=POSE):
    """w = t + R(theta)^T z."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return pose[0] + c * zx + s * zy, pose[1] - s * zx + c * zy


def stage(landmarks_z, tab, ev, scan, margin=0.3, bins=128, K=2):
    """One particle at POSE; landmarks at the sensor-frame points landmarks_z; scan: sensor-frame points (None: an all-inf table)."""
    L = len(landmarks_z)
    mp = np.zeros((1, 5, L), F)
    for l, (zx, zy) in enumerate(landmarks_z):
        mp[0, 0, l], mp[0, 1, l] = to_world(zx, zy)
    mp[0, 2] = 0.3
    x, y, th = (np.array([v], F) for v in POSE)
    T = np.full(bins, np.inf, F) if scan is None else S.table(np.array([p[0] for p in scan], F), np.array([p[1] for p in scan], F), bins)
    a = (mp, x, y)
    b = (None, np.array([tab], np.uint8), K, np.array([ev], np.uint8), HIT, MISS, CMAX, RANGE)
    return S.evidence(*a, th, *b, T, margin), E.evidence(*a, *b)


def test_an_empty_table_is_the_plain_stage(orc):
    rng = np.random.default_rng(4)
    n, L = 7, 21
    mp = (rng.standard_normal((n, 5, L + 3)) * 3).astype(F)
    mp[:, 2][rng.random((n, L + 3)) < 0.3] = -1.0
    mp[0, 0, 0] = np.nan
    x, y, th = ((rng.standard_normal(n)).astype(F) for _ in range(3))
    tab = rng.choice(np.array([0, 1, 2, 255], np.uint8), (n, L + 1))
    ev = rng.integers(0, CMAX + 1, (n + 2, L + 2)).astype(np.uint8)
    anc = rng.integers(0, n + 2, n)
    for in_place in (False, True):
        a = None if in_place else anc
        got = S.evidence(mp, x, y, th, a, tab, 2, ev, HIT, MISS, CMAX, 4.0, np.full(64, np.inf, F), 0.3, L=L, in_place=in_place)
        want = E.evidence(mp, x, y, a, tab, 2, ev, HIT, MISS, CMAX, 4.0, L=L, in_place=in_place)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes() and np.array_equal(got[2], want[2])
        assert got[2][:, 0].sum() > 0 and np.all(got[3] == 0)


def test_hidden_hit_near_and_own_pole(orc):
    lm = [(4.0, 0.6), (4.0, 0.6), (0.2, 0.1), (-3.0, 1.0), (1.0, -3.0)]
    scan = [(2.0, 0.3),                            # in front of landmarks 0 and 1
            (0.05, 0.025),                         # in front of landmark 2, which is nearer than the margin
            (-3.0 * (1 - 0.1 / np.hypot(3, 1)), 1.0 * (1 - 0.1 / np.hypot(3, 1)))]   # landmark 3's own pole: a return at r - 0.1
    tab, ev = [255, 1, 255, 255, 255], [0, 3, 0, 0, 0]
    (mp, out, st, spared), (mp0, out0, st0) = stage(lm, tab, ev, scan)
    # plain: 0, 2, 3 and 4 cannot pay the miss and are pruned; 1 is hit
    assert out0.tolist() == [[0, 5, 0, 0, 0]] and st0.tolist() == [[4, 1]]
    # sight: 0 is hidden and keeps its slot; 1 is hidden and its hit still counts; 2 (g <= 0), 3 (its own pole) and 4 (nothing there) take the miss
    assert out.tolist() == [[0, 5, 0, 0, 0]] and st.tolist() == [[3, 2]] and spared.tolist() == [1]
    assert mp[0, 2].tolist() == [F(0.3), F(0.3), -1.0, -1.0, -1.0] and mp[0, 0, 0] == mp0[0, 0, 1]
    w = np.array([to_world(*z) for z in lm], F)
    hid, _, has = S.hidden(S.table(np.array([p[0] for p in scan], F), np.array([p[1] for p in scan], F), 128), 0.3,
                           *(np.array([v], F) for v in POSE), w[None, :, 0], w[None, :, 1])
    assert hid.tolist() == [[True, True, False, False, False]] and has.all()
    # a margin below the pole's radius: landmark 3's own pole hides it (why the margin is there), and landmark 2 is no longer too near
    (_, out, _, spared), _ = stage(lm, tab, ev, scan, margin=0.05)
    assert spared.tolist() == [3] and out.tolist() == [[0, 5, 0, 0, 0]]
    # the neighbour window: a return one bin to either side hides, two bins away does not
    def along(q, r):   # the point of the first quadrant with |y| / (|x| + |y|) = q at range r
        return tuple(r * np.array([1 - q, q]) / np.hypot(1 - q, q))
    for d, want in ((0, 1), (1, 1), (-1, 1), (2, 0), (-2, 0)):
        lz, sz = along(16.5 / 32, 4.5), along((16.5 + d) / 32, 2.0)   # 128 bins: 32 equal steps of q per quadrant; mid-bin
        jl, js = one_bin(*lz, 128), one_bin(*sz, 128)
        (_, _, _, spared), _ = stage([lz], [255], [5], [sz])
        assert jl == 16 and js - jl == d and spared.tolist() == [want], (d, js, jl)
