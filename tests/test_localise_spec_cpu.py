"""tests/_localise_spec.py on the CPU: the composition the GPU stage is held to.  Its log-likelihood is the textbook Gaussian
likelihood of the matched pairs (float64), the table never names a slot without a landmark, nothing is ever created, and the
clutter term decides between a particle that explains nothing and one that explains everything."""
import numpy as np
import pytest

import _assoc_spec as A
import _localise_spec as S
from _localise_bounds import textbook, within

F = np.float32
Q, GATE = 0.02, 9.21
# two landmarks with det (P + q I) > 1 (a pair's term is then negative whatever its Mahalanobis distance), and an empty slot between them
M = np.array([[5.0, 0.0, 0.0], [0.0, 0.0, 5.0], [1.2, -1.0, 1.5], [0.3, 0.0, -0.2], [1.0, 0.0, 0.9]], np.float32)
POSE = (0.2, -0.1, 0.3)


def sense(points, pose):
    """z = H (m - t), H = [[c, -s], [s, c]] (float64): the sensor-frame points a pose sees world points at."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    dx, dy = points[:, 0] - pose[0], points[:, 1] - pose[1]
    return c * dx - s * dy, s * dx + c * dy


@pytest.fixture(scope="module")
def case(orc):
    zx, zy = sense(np.array([[5.0, 0.0], [0.0, 5.0]]), POSE)
    zx, zy = (zx + [0.15, -0.2]).astype(F), (zy + [-0.1, 0.25]).astype(F)
    # particle 0 sits on the pose and matches both; particle 1 is far away and matches nothing
    x, y, th = np.array([POSE[0], 40.0], F), np.array([POSE[1], 40.0], F), np.array([POSE[2], 1.0], F)
    return x, y, th, zx[::-1].copy(), zy[::-1].copy()   # (detection 0 belongs to landmark 2, detection 1 to landmark 0)


def test_loglik_is_the_textbook_likelihood(case):
    x, y, th, zx, zy = case
    assoc, stats, ll = S.localise(M, x, y, th, zx, zy, Q, GATE, 0.0)
    assert assoc[0].tolist() == [1, A.NONE, 0] and stats[0].tolist() == [2, 0, 0]
    want = textbook(M, Q, x[0], y[0], th[0], zx, zy, [(0, 1), (2, 0)])
    assert within(ll[0], want), (ll[0], want)
    assert assoc[1].tolist() == [A.NONE] * 3 and stats[1].tolist() == [0, 0, 2]


def test_never_an_unseen_slot_and_nothing_created(orc):
    rng = np.random.default_rng(3)
    L, n, K = 70, 50, 12
    Mr = np.zeros((5, L), np.float32)
    Mr[0], Mr[1] = rng.uniform(-6, 6, L), rng.uniform(-6, 6, L)
    Mr[2], Mr[4] = 0.05, 0.08
    unseen = rng.random(L) < 0.4
    Mr[2, unseen] = -1.0
    x, y, th = (0.3 * rng.standard_normal(n)).astype(F), (0.3 * rng.standard_normal(n)).astype(F), (0.05 * rng.standard_normal(n)).astype(F)
    # detections ON the empty slots' stale means as well as on landmarks: the former must stay unmatched
    pick = np.concatenate([np.flatnonzero(unseen)[:6], np.flatnonzero(~unseen)[:6]])
    zx, zy = Mr[0, pick].copy(), Mr[1, pick].copy()
    assoc, stats, ll = S.localise(Mr, x, y, th, zx, zy, Q, 25.0, -1.0)
    assert np.all(assoc[:, unseen] == A.NONE)
    assert stats[:, 0].sum() > 0 and np.all(stats[:, 1] == 0) and np.all(stats.sum(axis=1) == K)
    assert np.array_equal(stats[:, 0], (assoc != A.NONE).sum(axis=1))


def test_the_clutter_term_decides(case):
    x, y, th, zx, zy = case
    _, _, ll = S.localise(M, x, y, th, zx, zy, Q, GATE, 0.0)
    assert ll[1] == 0 and ll[0] < ll[1]            # explaining nothing costs nothing: the lost particle outweighs the right one
    _, stats, llc = S.localise(M, x, y, th, zx, zy, Q, GATE, -5.0)
    assert llc[1] == F(-10.0) and llc[0] == ll[0] and llc[0] > llc[1]   # two unexplained detections at -5 each: it no longer does
    with pytest.raises(ValueError):
        S.localise(M, x, y, th, zx, zy, Q, GATE, 0.5)
