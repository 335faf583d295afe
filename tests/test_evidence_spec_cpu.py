"""tests/_evidence_spec.py against hand-worked answers, each case on the edge it names.  No GPU."""
import numpy as np

import _assoc_spec as A
import _evidence_spec as E
from conftest import bits

F = np.float32
NONE = A.NONE


def one(mx=1.0, my=1.0, pxx=0.5, c=4, a=NONE, K=3, hit=1, miss=1, cmax=8, view_range=5.0, px=0.0, py=0.0):
    """One particle with one landmark -> (c', pruned, the slot's five planes, stats)."""
    row = np.array([[[mx], [my], [pxx], [0.25], [0.75]]], np.float32)
    mp, ev, st = E.evidence(row, [px], [py], None, np.array([[a]], np.uint8), K, np.array([[c]], np.uint8), hit, miss, cmax, view_range)
    return int(ev[0, 0]), bool(st[0, 0]), mp[0, :, 0], st[0]


def fresh(planes):
    return np.array_equal(bits(planes), bits(np.array([0.0, 0.0, -1.0, 0.0, 0.0], np.float32)))


def test_miss_edges():
    c, pruned, planes, st = one(c=2, miss=3)          # c == miss - 1: cannot pay
    assert (c, pruned) == (0, True) and fresh(planes) and list(st) == [1, 0]
    c, pruned, planes, st = one(c=3, miss=3)          # c == miss: pays with its last evidence, stays
    assert (c, pruned) == (0, False) and not fresh(planes) and list(st) == [0, 1]
    assert np.array_equal(planes, np.array([1.0, 1.0, 0.5, 0.25, 0.75], np.float32))
    assert one(c=7, miss=3)[:2] == (4, False)
    assert one(c=0, miss=1)[:2] == (0, True)


def test_hit_is_clamped_in_integers():
    assert one(c=6, hit=3, cmax=8, a=0)[0] == 8       # 9 -> cmax
    assert one(c=5, hit=3, cmax=8, a=0)[0] == 8       # exactly cmax
    assert one(c=4, hit=3, cmax=8, a=0)[0] == 7
    assert one(c=200, hit=255, cmax=255, a=0)[0] == 255   # 455 must not wrap to 199
    assert one(c=200, hit=255, cmax=100, a=0)[0] == 100   # (an evidence above a lowered cmax comes down to it)
    assert one(c=0, hit=1, cmax=8, a=2, K=3)[:2] == (1, False)


def test_visibility_edge():
    assert one(mx=3.0, my=4.0, c=4)[0] == 3                                   # r2 == range2 == 25: visible, a miss
    up = float(np.nextafter(F(3.0), F(4.0)))
    assert one(mx=up, my=4.0, c=4)[0] == 4                                    # the next float32 above 3: r2 = 25.000002, not visible
    assert one(mx=up, my=4.0, c=0)[:2] == (0, False)                          # ... so not pruned either
    assert one(mx=3.0 + 10.0, my=4.0 - 2.0, px=10.0, py=-2.0, c=4)[0] == 3    # relative to the pose
    # range2 is rounded once: 0.1f * 0.1f = 0.010000001f, and dx = 0.1f, dy = 0 gives the same product
    assert one(mx=float(F(0.1)), my=0.0, view_range=0.1, c=4)[0] == 3


def test_nan_and_inf_means():
    for mx, my in ((np.nan, 1.0), (1.0, np.nan), (np.inf, 1.0), (1.0, -np.inf), (np.inf, np.inf)):
        c, pruned, planes, _ = one(mx=mx, my=my, c=0)
        assert (c, pruned) == (0, False) and not fresh(planes)                # not visible: never a miss, never pruned
        assert one(mx=mx, my=my, c=5)[0] == 5
        assert one(mx=mx, my=my, c=5, a=1)[0] == 6                            # a hit does not ask for visibility


def test_seen_is_the_updates_own_test():
    assert one(pxx=-0.0, c=4)[0] == 3                                         # -0.0 is not < 0: seen, a miss
    c, pruned, planes, st = one(pxx=-0.0, c=0)
    assert pruned and fresh(planes)
    c, pruned, planes, st = one(pxx=-1.0, c=7, a=0)                           # not seen: 0 whatever the table says
    assert (c, pruned) == (0, False) and list(st) == [0, 0]
    assert one(pxx=float(np.nextafter(F(0), F(-1))), c=7)[0] == 0             # the smallest negative value: unseen
    assert one(pxx=np.nan, c=4)[0] == 3                                       # NaN is not < 0: seen


def test_table_bytes_that_name_no_detection():
    for a in (3, 10, 63):                                                     # K <= a < 64
        assert one(a=a, K=3, c=4)[0] == 3
    for a in (64, 100, 254, 255):                                             # 64 .. 254 and SLAM_ASSOC_NONE
        assert one(a=a, K=64, c=4)[0] == 3
    assert one(a=63, K=64, c=4)[0] == 5
    assert one(a=2, K=3, c=4)[0] == 5


def test_no_detections_is_an_observing_frame():
    for a in (0, 5, NONE):
        assert one(a=a, K=0, c=4)[0] == 3                                     # K = 0: nothing is a hit, the visible take a miss
    assert one(a=0, K=0, c=4, mx=30.0)[0] == 4
    assert one(a=0, K=0, c=0)[1]


def test_init_padding_and_strides():
    mp = np.zeros((3, 5, 8), np.float32)
    mp[:, 2] = [[0.5, -1.0, -0.0, np.nan, -2.0, 0.0, 1.0, -1.0]] * 3
    ev = E.evidence_init(mp, 9, L=6, ev_stride=7)
    assert ev.dtype == np.uint8 and np.array_equal(ev, [[9, 0, 9, 9, 0, 9, 0]] * 3)
    assert np.array_equal(E.evidence_init(mp, 0, L=8), np.zeros((3, 8), np.uint8))
    # out of place the padding columns are written 0, in place they are left alone; the row's padding is never touched
    mp[:, :2] = 1.0
    ev_in = np.full((3, 7), 5, np.uint8)
    tab = np.full((3, 8), NONE, np.uint8)
    out_mp, out, st = E.evidence(mp, np.zeros(3, F), np.zeros(3, F), None, tab, 1, ev_in, 1, 6, 8, 5.0, L=6)
    assert np.array_equal(out, [[0, 0, 0, 0, 0, 0, 0]] * 3) and np.array_equal(st, [[4, 0]] * 3)
    assert np.array_equal(bits(out_mp[:, :, 6:]), bits(mp[:, :, 6:]))
    assert np.array_equal(out_mp[0, 2, :6], [-1.0, -1.0, -1.0, -1.0, -2.0, -1.0]) and np.all(   # (an unseen slot keeps its own bits)
out_mp[0, [0, 1, 3, 4], :6][:, [0, 2, 3, 5]] == 0)
    _, out, _ = E.evidence(mp, np.zeros(3, F), np.zeros(3, F), None, tab, 1, ev_in, 1, 1, 8, 5.0, L=6, in_place=True)
    assert np.array_equal(out, [[4, 0, 4, 4, 0, 4, 5]] * 3)


def test_duplicate_ancestors_read_the_same_evidence_row():
    n, L = 4, 3
    mp = np.ones((n, 5, L), np.float32)
    ev_in = np.array([[1, 2, 3], [4, 5, 6], [7, 7, 7], [0, 0, 0]], np.uint8)
    tab = np.array([[0, NONE, NONE]] * n, np.uint8)
    anc = np.array([1, 1, 3, 1], np.int32)
    _, out, st = E.evidence(mp, np.zeros(n, F), np.zeros(n, F), anc, tab, 1, ev_in, 2, 1, 8, 5.0)
    assert np.array_equal(out, [[6, 4, 5], [6, 4, 5], [2, 0, 0], [6, 4, 5]])   # the MAP row is the particle's own, the evidence its ancestor's
    assert np.array_equal(st, [[0, 3], [0, 3], [2, 1], [0, 3]])
    assert np.array_equal(ev_in, [[1, 2, 3], [4, 5, 6], [7, 7, 7], [0, 0, 0]])


def test_a_pruned_slot_is_a_fresh_slot_and_is_handed_out_again(orc):
    """Two slots, one holds a landmark nobody detects: pruned, bit-identical to a slot never used, and the next frame's
    association starts a new landmark in it."""
    mp = np.zeros((1, 5, 2), np.float32)
    mp[0, :, 0] = [2.0, 0.0, 0.01, 0.0, 0.01]
    mp[0, :, 1] = [-2.0, 1.0, 0.01, 0.0, 0.01]
    x = y = th = np.zeros(1, F)
    zx, zy = np.array([2.0], F), np.array([0.0], F)
    tab, _ = A.associate(mp, x, y, th, None, zx, zy, 0.01, 9.21, 50.0, 1)
    assert list(tab[0]) == [0, NONE]
    mp1, _ = A.update(mp, x, y, th, None, tab, zx, zy, 0.01)
    mp2, ev, st = E.evidence(mp1, x, y, None, tab, 1, np.array([[1, 0]], np.uint8), 1, 1, 8, 9.0)
    assert list(ev[0]) == [2, 0] and list(st[0]) == [1, 1]
    never = np.zeros((5,), np.float32)
    never[2] = -1.0
    assert np.array_equal(bits(mp2[0, :, 1]), bits(never)) and np.array_equal(bits(mp2[0, :, 0]), bits(mp1[0, :, 0]))
    zx, zy = np.array([2.0, -3.0], F), np.array([0.0, -4.0], F)
    tab, ast = A.associate(mp2, x, y, th, None, zx, zy, 0.01, 9.21, 50.0, 1)
    assert list(tab[0]) == [0, 1] and list(ast[0]) == [1, 1, 0]                 # matched, created in the pruned slot, none dropped
