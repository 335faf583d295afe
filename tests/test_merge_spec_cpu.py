"""tests/_merge_spec.py by itself: every branch of the merge rule on hand-made rows, and the fusion against the float64
information-form product (P_w^-1 + P_l^-1)^-1.

The float64 bounds (u = 2^-24; S = P_l + P_w with eigenvalues lambda_min(S) <= lambda_max(S), kappa(S) their ratio; d = mu_l -
mu_w; the inputs are float32 values and exact), derived as tests/test_aniso_spec_cpu.py derives those of the general-covariance
update, whose arithmetic this is with the observed point w = mu_l (exact here: no pose, no sine) and the noise R = P_l:

  mean        |mu' - mu'_64| <= a u |d| + 2 u (|mu_l| + |d|) + u (6 kappa(S) + 18) lambda_max(P_l) |d| / lambda_min(S)
              a = max(1, ||P_l S^-1||_2): the rounding of d (u |d|) passes through P_l S^-1; the last subtraction and the
              product's sum; the roundings of S, of det S and its reciprocal ((2 kappa(S) + 2) u), of S^-1 d and of P_l (S^-1 d),
              all through ||P_l|| ||S^-1|| <= lambda_max(P_l) / lambda_min(S).
  covariance  max |P'_ij - P'_64,ij| <= 4 u ((kappa(S) + 2) lambda_max(P')
                                             + (lambda_max(P_l) (w_xx w_yy + w_xy^2) + lambda_max(P_w) (l_xx l_yy + l_xy^2)) / det S)
              the update's bound with BOTH determinants rounded (there det Q is an input): each is a difference of two rounded
              products, 2 u (p_xx p_yy + p_xy^2), and multiplies the other matrix over det S.
"""
import numpy as np
import pytest

import _merge_cases as MC
import _merge_spec as M
from _merge_bounds import fusion_check

F = np.float32
U = 2.0 ** -24
GATE = 9.0


def row(*slots, stride=None):
    """slots: (mu_x, mu_y, P_xx, P_xy, P_yy) per landmark -> [1][5][stride]."""
    L = len(slots)
    mp = np.full((1, 5, stride or L), np.nan, F)
    mp[0, :, :L] = np.array(slots, F).T
    return mp


def run(slots, bytes_, K=4, ev=None, cmax=None, gate=GATE, stride=None):
    mp = row(*slots, stride=stride)
    tab = np.array([bytes_], np.uint8)
    e = None if ev is None else np.array([ev], np.uint8)
    out, ev_out, st = M.merge(mp, tab, K, gate, e, cmax, L=len(slots))
    return mp, out, ev_out, st[0].tolist()


ANCHOR = (1.0, 2.0, 0.5, 0.0, 0.5)
DUP = (1.05, 1.97, 0.05, 0.01, 0.04)
FRESH = np.array(M.FRESH, F)


def test_a_duplicate_is_fused_and_its_slot_cleared():
    mp, out, ev, st = run([ANCHOR, DUP], [0, 255], ev=[3, 4], cmax=8, stride=4)
    assert st == [1, 0, 1]
    want = np.array(M.fuse(tuple(mp[0, :, 1]), tuple(mp[0, :, 0])), F)
    assert out[0, :, 0].tobytes() == want.tobytes() and out[0, :, 1].tobytes() == FRESH.tobytes()
    assert ev[0].tolist() == [7, 0]
    assert out[0, :, 2:].tobytes() == mp[0, :, 2:].tobytes()          # the padding columns
    # the fused estimate lies between the two and is tighter than either
    assert 1.0 < out[0, 0, 0] < 1.05 and 1.97 < out[0, 1, 0] < 2.0 and out[0, 2, 0] < 0.05 and out[0, 4, 0] < 0.04


def test_evidence_saturates_at_cmax_in_integers():
    assert run([ANCHOR, DUP], [0, 255], ev=[200, 255], cmax=255)[2][0].tolist() == [255, 0]
    assert run([ANCHOR, DUP], [0, 255], ev=[6, 5], cmax=8)[2][0].tolist() == [8, 0]
    assert run([ANCHOR, DUP], [0, 255], ev=[0, 0], cmax=8)[2][0].tolist() == [0, 0]
    assert run([ANCHOR, DUP], [0, 255])[2] is None


def test_roles():
    # unseen slots, far slots and slots beyond the gate stay; a byte >= K names nothing (the slot is free, not an anchor)
    far = (1.0, 500.0, 0.05, 0.0, 0.05)
    unseen = (1.0, 2.0, -1.0, 0.0, 0.0)
    mp, out, _, st = run([ANCHOR, far, unseen], [1, 255, 255])
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([ANCHOR, DUP], [4, 255])                      # K = 4: byte 4 is no anchor
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([ANCHOR, DUP], [0, 5])                        # ... and byte 5 makes the duplicate no anchor: merged
    assert st == [1, 0, 1]
    mp, out, _, st = run([ANCHOR, DUP], [0, 255], K=0)                 # no detections: no anchors
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([unseen[:2] + (-1.0, 0.0, 0.0), DUP], [0, 255])   # a named slot that is unseen is no anchor
    assert st == [0, 0, 1] and out.tobytes() == mp.tobytes()


def test_two_anchors_at_one_point_are_not_merged():
    mp, out, _, st = run([ANCHOR, ANCHOR], [0, 1])
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()


def test_just_inside_and_just_outside_the_gate():
    m = float(M.pair_cost(tuple(F(v) for v in DUP), tuple(F(v) for v in ANCHOR)))
    assert run([ANCHOR, DUP], [0, 255], gate=m)[3] == [1, 0, 1]       # m == gate: a candidate
    assert run([ANCHOR, DUP], [0, 255], gate=float(np.nextafter(F(m), F(0))))[3] == [0, 0, 2]


def test_two_free_landmarks_choose_one_anchor():
    near, farther = DUP, (1.1, 2.1, 0.05, 0.01, 0.04)
    for slots, bytes_, absorbed, waits in (([ANCHOR, near, farther], [0, 255, 255], 1, 2), ([farther, near, ANCHOR], [255, 255, 2], 1, 0)):
        mp, out, _, st = run(slots, bytes_)
        assert st == [1, 0, 2]
        assert out[0, :, absorbed].tobytes() == FRESH.tobytes() and out[0, :, waits].tobytes() == mp[0, :, waits].tobytes()
    # ... the one that waited is absorbed by the next frame's stage
    mp, out, _, st = run([ANCHOR, near, farther], [0, 255, 255])
    out2, _, st2 = M.merge(out, np.array([[0, 255, 255]], np.uint8), 4, GATE)
    assert st2[0].tolist() == [1, 0, 1] and out2[0, :, 2].tobytes() == FRESH.tobytes()


def test_ties():
    # the same cost at one anchor: the lowest l is absorbed (m = 0 for both: -0 and +0 are one value)
    mp, out, _, st = run([ANCHOR, ANCHOR, ANCHOR], [255, 0, 255])
    assert st == [1, 0, 2] and out[0, :, 0].tobytes() == FRESH.tobytes() and out[0, :, 2].tobytes() == mp[0, :, 2].tobytes()
    # the same cost at two anchors: the free landmark chooses the lowest w, the other anchor is chosen by none
    a0, a1, mid = (0.0, 0.0, 0.5, 0.0, 0.5), (1.0, 0.0, 0.5, 0.0, 0.5), (0.5, 0.0, 0.5, 0.0, 0.5)
    for slots, bytes_, chosen, other in (([a0, mid, a1], [2, 255, 3], 0, 2), ([mid, a1, a0], [255, 0, 1], 1, 2)):
        mp, out, _, st = run(slots, bytes_)
        assert st == [1, 0, 2]
        assert out[0, :, other].tobytes() == mp[0, :, other].tobytes() and out[0, :, chosen].tobytes() != mp[0, :, chosen].tobytes()


def test_nan_minus_zero_and_singular():
    nan = float("nan")
    for bad in ((nan, 2.0, 0.05, 0.0, 0.05), (1.0, nan, 0.05, 0.0, 0.05), (1.0, 2.0, 0.05, nan, 0.05)):
        mp, out, _, st = run([ANCHOR, bad], [0, 255])
        assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([(nan, 2.0, 0.5, 0.0, 0.5), DUP], [0, 255])   # a NaN anchor absorbs nothing
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    # -0.0 in P_xx is seen (the update's own test) and takes part: a candidate — whose fused P_xx is no more than 0: refused
    mp, out, _, st = run([ANCHOR, (1.01, 2.0, -0.0, 0.0, 0.04)], [0, 255])
    assert st == [0, 1, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([ANCHOR, (1.01, 2.0, -0.0, 0.0, 0.04)], [255, 0])   # ... and as an anchor it is one
    assert st == [0, 1, 2] and out.tobytes() == mp.tobytes()
    # S singular: det S = 0, every cost NaN or infinite, no candidate
    flat = (1.0, 2.0, 1.0, 1.0, 1.0)
    mp, out, _, st = run([flat, (1.5, 2.0, 1.0, 1.0, 1.0)], [0, 255])
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()
    mp, out, _, st = run([(1.0, 2.0, 0.0, 0.0, 0.0), (1.0, 2.0, 0.0, 0.0, 0.0)], [0, 255])
    assert st == [0, 0, 2] and out.tobytes() == mp.tobytes()


def test_the_guard_refuses_and_writes_nothing():
    # a free landmark on the anchor (m = 0) whose covariance is not positive definite: the fused P_xx would be negative
    bad = (1.0, 2.0, 0.05, 0.2, 0.05)
    mp, out, ev, st = run([ANCHOR, bad], [0, 255], ev=[3, 4], cmax=8)
    o = M.fuse(tuple(mp[0, :, 1]), tuple(mp[0, :, 0]))
    assert o[2] < 0 and not M.guard(o)
    assert st == [0, 1, 2] and out.tobytes() == mp.tobytes() and ev[0].tolist() == [3, 4]
    # each clause of the guard
    ok = (F(1), F(2), F(0.1), F(0.01), F(0.1))
    assert M.guard(ok)
    for j, v in ((0, np.inf), (1, np.nan), (2, 0.0), (2, -0.1), (4, 0.0), (3, 0.1), (3, 0.2), (2, np.inf), (3, -np.inf)):
        o = list(ok)
        o[j] = F(v)
        assert not M.guard(tuple(o)), (j, v)
    # an overflowing fusion is refused: covariances near the top of the range
    big = 3e38
    mp, out, _, st = run([(0.0, 0.0, big, 0.0, big), (0.0, 0.0, big, 0.0, big)], [0, 255])
    assert st[0] == 0 and out.tobytes() == mp.tobytes()


def test_more_than_64_named_slots():
    """A table that names a detection twice: the first 64 named slots in ascending l are the anchors, the others take no part."""
    L = 70
    slots = [(4.0 * l, 0.0, 0.5, 0.0, 0.5) for l in range(L)]
    slots[69] = (4.0 * 66 + 0.05, 0.0, 0.05, 0.0, 0.05)               # beside slot 66, which is named but behind the 64th
    slots[68] = (4.0 * 3 + 0.05, 0.0, 0.05, 0.0, 0.05)                # beside slot 3, an anchor
    mp, out, _, st = run(slots, [l % 4 for l in range(68)] + [255, 255])
    assert st == [1, 0, 69] and out[0, :, 68].tobytes() == FRESH.tobytes() and out[0, :, 69].tobytes() == mp[0, :, 69].tobytes()
    assert out[0, :, 4:68].tobytes() == mp[0, :, 4:68].tobytes()


@pytest.mark.parametrize("anchors,K", [(0, 4), (1, 1), (4, 4), (8, 64), (64, 64)])
def test_the_shared_cases_hold_every_branch(anchors, K):
    """The rows of _merge_cases.py (what the GPU test places per particle): what each kind of slot must come to."""
    n, L = 13, 200
    mp, tab, c, kind = MC.make_case(n, L, 224, K, anchors, seed=anchors + K)
    out, ev, st = M.merge(mp, tab, K, GATE, c, 200, L=L)
    cleared = (out[:, 2, :L] < 0) & ~(mp[:, 2, :L] < 0)
    assert np.array_equal(st[:, 0], cleared.sum(axis=1)) and out[:, :, L:].tobytes() == mp[:, :, L:].tobytes()
    seen_after = (~(out[:, 2, :L] < 0)).sum(axis=1)
    assert np.array_equal(st[:, 2], seen_after)
    if anchors == 0:
        assert st[:, :2].sum() == 0 and out.tobytes() == mp.tobytes() and ev.tobytes() == c.tobytes()
        return
    for k in (2, 3, 4, 5, 8):                                         # far away, unseen, NaN mean, P_xx = -0.0, singular S: never absorbed
        assert not cleared[kind == k].any(), MC.KINDS[k]
    assert not cleared[kind == -1].any() and st[:, 0].max() <= min(anchors, K)
    assert st[:, 0].sum() > 0
    if anchors >= 4:
        for k in (6,) + ((0, 10, 11) if anchors == 64 else ()):           # (few anchors: one "on the anchor" always beats a duplicate)
            assert cleared[kind == k].any(), MC.KINDS[k]
        assert anchors < 8 or st[:, 1].sum() > 0                      # the guard refused a "not positive definite" somewhere
        assert (ev[:, :L][~cleared & (kind == -1)] == 200).any()      # an anchor's evidence saturated
    # no anchor was turned into an unused slot or into garbage
    anchor_vals = np.moveaxis(out[:, :, :L], 1, 2)[kind == -1]
    assert np.all(np.isfinite(anchor_vals)) and np.all(anchor_vals[:, 2] >= 0)
    assert np.all(ev[:, :L][cleared] == 0)


def regimes(n, seed):
    """Pairs (P_l, P_w) over condition numbers 1 .. 1e4, relative sizes 1e-3 .. 1e3 and scales 1e-6 .. 1e2; d within a few sigma."""
    rng = np.random.default_rng(seed)

    def spd(lmax, kappa):
        a = rng.uniform(0, np.pi, n)
        l1, l2 = lmax, lmax / kappa
        c, s = np.cos(a), np.sin(a)
        return np.stack([l1 * c * c + l2 * s * s, (l1 - l2) * c * s, l1 * s * s + l2 * c * c]).astype(F)

    scale = 10.0 ** rng.uniform(-6, 2, n)
    pl = spd(scale, 10.0 ** rng.uniform(0, 4, n))
    pw = spd(scale * 10.0 ** rng.uniform(-3, 3, n), 10.0 ** rng.uniform(0, 4, n))
    mw = rng.uniform(-1e3, 1e3, (2, n)).astype(F)
    sig = np.sqrt(np.maximum(pl[0] + pw[0], pl[2] + pw[2]).astype(np.float64))
    ml = (mw + rng.standard_normal((2, n)) * 2 * sig).astype(F)
    return ml, pl, mw, pw


def test_fusion_within_its_bounds_of_the_float64_product():
    n = 20000
    ml, pl, mw, pw = regimes(n, 11)
    with np.errstate(all="ignore"):
        o = np.array(M.fuse((ml[0], ml[1], pl[0], pl[1], pl[2]), (mw[0], mw[1], pw[0], pw[1], pw[2])), np.float64)
    fusion_check(o, ml, pl, mw, pw)
