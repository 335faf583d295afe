"""tests/_assoc_spec.py (the specification of data association) on the CPU: it recovers the identities of a well separated scene,
feeds the update what the known-correspondence oracle gets, never uses a detection or a landmark twice, does not care about the
order of the detections, creates landmarks in slot order and drops what does not fit, and agrees with a float64 brute force
wherever that one's decision is not a matter of rounding."""
import numpy as np
import pytest

import _assoc_spec as A
from conftest import bits

Q, GATE, NEW_GATE = 1e-3, 9.21, 50.0


def scene(n=48, L=24, seed=3, min_sep=2.0, unseen=0):
    """Landmarks at least min_sep apart, particles around the origin whose maps hold the truth blurred by a few centimetres
    (P = 0.05^2 I and a little correlation); the detections are the exact observations from a reference pose every particle is
    within centimetres of.  -> poses, rows [n][5][L], lm [L][2], (zx, zy) in landmark order."""
    rng = np.random.default_rng(seed)
    lm = []
    while len(lm) < L:
        p = rng.uniform(-20, 20, 2)
        if all(np.hypot(*(p - o)) >= min_sep for o in lm):
            lm.append(p)
    lm = np.array(lm, np.float32)
    x = (0.01 * rng.standard_normal(n)).astype(np.float32)
    y = (0.01 * rng.standard_normal(n)).astype(np.float32)
    th = (0.3 + 0.0005 * rng.standard_normal(n)).astype(np.float32)
    rows = np.empty((n, 5, L), np.float32)
    rows[:, 0] = lm[:, 0] + 0.02 * rng.standard_normal((n, L))
    rows[:, 1] = lm[:, 1] + 0.02 * rng.standard_normal((n, L))
    rows[:, 2] = 0.0025
    rows[:, 3] = 0.0005 * rng.standard_normal((n, L))
    rows[:, 4] = 0.0025
    if unseen:
        rows[:, 2, L - unseen:] = -1.0
    c, s = np.cos(0.3), np.sin(0.3)
    zx = (c * lm[:, 0] - s * lm[:, 1]).astype(np.float32)      # z = H m for the pose (0, 0, 0.3), H = [[c, -s], [s, c]] (slam_hip.h)
    zy = (s * lm[:, 0] + c * lm[:, 1]).astype(np.float32)
    return (x, y, th), rows, lm, (zx, zy)


@pytest.fixture(scope="module")
def case(orc):
    (x, y, th), rows, lm, (zx, zy) = scene()
    perm = np.random.default_rng(8).permutation(len(lm))
    assoc, stats = A.associate(rows, x, y, th, None, zx[perm], zy[perm], Q, GATE, NEW_GATE, 1)
    return dict(x=x, y=y, th=th, rows=rows, zx=zx, zy=zy, perm=perm, assoc=assoc, stats=stats)


def test_every_identity_is_recovered(case):
    L = len(case["perm"])
    inv = np.argsort(case["perm"])          # landmark l was observed as detection inv[l]
    assert np.array_equal(case["assoc"], np.broadcast_to(inv.astype(np.uint8), case["assoc"].shape))
    assert np.array_equal(case["stats"], np.broadcast_to(np.array([L, 0, 0], np.int32), case["stats"].shape))


def test_updated_rows_equal_the_known_correspondence_update(case, orc):
    c = case
    rng = np.random.default_rng(5)
    anc = rng.integers(0, len(c["x"]), len(c["x"])).astype(np.int32)
    ids = np.arange(len(c["perm"]), dtype=np.int32)
    for a in (None, anc):
        assoc, _ = A.associate(c["rows"], c["x"], c["y"], c["th"], a, c["zx"][c["perm"]], c["zy"][c["perm"]], Q, GATE, NEW_GATE, 1)
        got, got_ll = A.update(c["rows"], c["x"], c["y"], c["th"], a, assoc, c["zx"][c["perm"]], c["zy"][c["perm"]], Q)
        want, want_ll = orc.ekf_update(c["rows"], c["x"], c["y"], c["th"], a, ids, c["zx"], c["zy"], Q)
        assert np.array_equal(bits(got), bits(want)) and np.array_equal(bits(got_ll), bits(want_ll))


def crowded(orc, seed=21, n=40, L=60, K=40):
    """A scene where association is contested: landmarks 0.3 m apart on average, wide priors, noisy detections, some clutter."""
    rng = np.random.default_rng(seed)
    lm = rng.uniform(-2, 2, (L, 2))
    x = (0.05 * rng.standard_normal(n)).astype(np.float32)
    y = (0.05 * rng.standard_normal(n)).astype(np.float32)
    th = rng.uniform(-3, 3, n).astype(np.float32)
    rows = np.empty((n, 5, L), np.float32)
    rows[:, 0] = lm[:, 0] + 0.1 * rng.standard_normal((n, L))
    rows[:, 1] = lm[:, 1] + 0.1 * rng.standard_normal((n, L))
    sx, sy, r = rng.uniform(0.05, 0.3, (n, L)), rng.uniform(0.05, 0.3, (n, L)), rng.uniform(-0.8, 0.8, (n, L))
    rows[:, 2], rows[:, 3], rows[:, 4] = sx * sx, r * sx * sy, sy * sy
    rows[:, 2][rng.random((n, L)) < 0.15] = -1.0
    z = np.concatenate([lm[rng.permutation(L)[:K - 8]] + 0.05 * rng.standard_normal((K - 8, 2)), rng.uniform(-4, 4, (8, 2))])
    return (x, y, th), rows, z[:, 0].astype(np.float32), z[:, 1].astype(np.float32)


def test_no_detection_twice_and_permutation_equivariance(orc):
    (x, y, th), rows, zx, zy = crowded(orc)
    K = len(zx)
    assoc, stats = A.associate(rows, x, y, th, None, zx, zy, 0.01, GATE, NEW_GATE, 1)
    assert 0 < stats[:, 0].min() and stats[:, 0].max() < K and stats[:, 1].max() > 0       # contested: neither trivial case
    for row, st in zip(assoc, stats):
        used = row[row != A.NONE]
        assert len(np.unique(used)) == len(used) and len(used) == st[0] + st[1] and st.sum() == K
    # create = 0: the matches are the same, nothing else is set; permuting the detections permutes the values of the matches
    # (e. hands the unseen slots out in order of k, so the creations are compared with create = 0)
    plain, pst = A.associate(rows, x, y, th, None, zx, zy, 0.01, GATE, NEW_GATE, 0)
    assert np.all(pst[:, 1] == 0) and np.array_equal(pst[:, 0], stats[:, 0])
    seen = ~(rows[:, 2] < 0)
    assert np.array_equal(plain[seen], assoc[seen]) and np.all(plain[~seen] == A.NONE)
    perm = np.random.default_rng(2).permutation(K)                 # new detection j is old detection perm[j]
    shuffled, sst = A.associate(rows, x, y, th, None, zx[perm], zy[perm], 0.01, GATE, NEW_GATE, 0)
    back = np.where(shuffled == A.NONE, A.NONE, perm[np.minimum(shuffled, K - 1)]).astype(np.uint8)
    assert np.array_equal(back, plain) and np.array_equal(sst, pst)
    # with creation the same holds for WHICH landmarks and how many (the new slots take the new detections in order of k)
    shuffled1, sst1 = A.associate(rows, x, y, th, None, zx[perm], zy[perm], 0.01, GATE, NEW_GATE, 1)
    assert np.array_equal(shuffled1 == A.NONE, assoc == A.NONE) and np.array_equal(sst1, stats)


def test_creation_fills_slots_in_order_and_drops_the_tail(orc):
    (x, y, th), rows, lm, (zx, zy) = scene(n=5, L=8)
    rows[:, 2] = -1.0                                                # nothing seen yet
    assoc, stats = A.associate(rows, x, y, th, None, zx, zy, Q, GATE, NEW_GATE, 1, assoc_stride=12)
    assert np.array_equal(assoc[:, :8], np.broadcast_to(np.arange(8, dtype=np.uint8), (5, 8))) and np.all(assoc[:, 8:] == A.NONE)
    assert np.all(stats == [0, 8, 0])
    none, nst = A.associate(rows, x, y, th, None, zx, zy, Q, GATE, NEW_GATE, 0)
    assert np.all(none == A.NONE) and np.all(nst == [0, 0, 8])      # create = 0 creates nothing
    assoc, stats = A.associate(rows[:, :, :5], x, y, th, None, zx, zy, Q, GATE, NEW_GATE, 1)   # 8 new detections, 5 slots
    assert np.array_equal(assoc, np.broadcast_to(np.arange(5, dtype=np.uint8), (5, 5))) and np.all(stats == [0, 5, 3])
    # a first sighting through the table is the update's own: mean = the observed point, P = q I, no likelihood term
    out, ll = A.update(rows[:, :, :5], x, y, th, None, assoc, zx, zy, Q)
    want, want_ll = orc.ekf_update(rows[:, :, :5], x, y, th, None, np.arange(5, dtype=np.int32), zx[:5], zy[:5], Q)
    assert np.array_equal(bits(out), bits(want)) and np.array_equal(bits(ll), bits(want_ll)) and np.all(ll == 0)


def brute_force_f64(rows, x, y, th, zx, zy, q):
    """Float64, libm: the cost of every (particle, landmark, detection) -> m [n][L][K], seen [n][L]."""
    r = rows.astype(np.float64)
    c, s = np.cos(th.astype(np.float64))[:, None], np.sin(th.astype(np.float64))[:, None]
    wx = x[:, None] + c * zx[None] + s * zy[None]
    wy = y[:, None] + c * zy[None] - s * zx[None]
    a, b, d = r[:, 2] + q, r[:, 3], r[:, 4] + q
    det = a * d - b * b
    dx, dy = wx[:, None, :] - r[:, 0, :, None], wy[:, None, :] - r[:, 1, :, None]
    m = (d[..., None] * dx * dx - 2 * b[..., None] * dx * dy + a[..., None] * dy * dy) / det[..., None]
    return m, ~(r[:, 2] < 0)


def test_float64_brute_force_agrees_where_it_is_decided(orc):
    """The two steps of the rule in float64.  A landmark's choice (c) is DECIDED when its two cheapest detections differ by more
    than 1e-3 relative and its minimum is not within 1e-3 relative of the gate; an undecided landmark taints the two detections
    it may end up competing for, and with them every landmark that chose one of those.  A detection's choice (d) is decided when
    the two cheapest candidates that chose it differ by as much.  Wherever everything a table entry depends on is decided, the
    float32 spec must hold the same entry; at least 95 % of the (particle, landmark) pairs qualify."""
    (x, y, th), rows, zx, zy = crowded(orc, seed=33)
    q = 0.01
    assoc, _ = A.associate(rows, x, y, th, None, zx, zy, q, GATE, NEW_GATE, 0)
    m, seen = brute_force_f64(rows, x, y, th, zx, zy, np.float64(np.float32(q)))
    n, L, K = m.shape
    rank = np.argsort(m, axis=2, kind="stable")
    kstar, ksecond = rank[:, :, 0], rank[:, :, 1]
    best, second = np.take_along_axis(m, rank[:, :, :2], axis=2).transpose(2, 0, 1)
    rel = lambda lo, hi: (hi - lo) > 1e-3 * np.abs(hi)
    unsure = seen & ~(rel(best, second) & (np.abs(best - GATE) > 1e-3 * GATE))
    cand = seen & (best >= 0) & (best <= GATE)
    want = np.full((n, L), A.NONE, np.uint8)
    decided = np.ones((n, L), bool)
    for i in range(n):
        tainted = np.zeros(K, bool)             # detections an unsure landmark may or may not compete for
        tainted[kstar[i][unsure[i]]] = True
        tainted[ksecond[i][unsure[i]]] = True
        decided[i] = ~(seen[i] & tainted[kstar[i]])
        for k in range(K):
            ls = np.flatnonzero(cand[i] & (kstar[i] == k))
            if len(ls) == 0:
                continue
            costs = np.sort(best[i, ls])
            want[i, ls[np.argmin(best[i, ls])]] = k
            if len(ls) > 1 and not rel(costs[0], costs[1]):
                decided[i, ls] = False
    share = decided.mean()
    assert share >= 0.95, share
    assert np.array_equal(assoc[decided], want[decided]), np.flatnonzero(assoc[decided] != want[decided])
