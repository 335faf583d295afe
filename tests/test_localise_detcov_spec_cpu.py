"""tests/_localise_detcov_spec.py on the CPU: the composition the GPU stage is held to.  With Q_k = q I for every detection it
matches what the isotropic stage matches (the log-likelihood's bits are pinned as they are: the two forms round S^-1 differently),
it is the rows pair of tests/_assoc_detcov_spec.py run on n copies of the map, and log_clutter = 0 leaves the clutter step out."""
import numpy as np
import pytest

import _assoc_detcov_spec as AD
import _assoc_weight_spec as W
import _localise_detcov_spec as SD
import _localise_spec as S
from conftest import bits

F = np.float32
Q, GATE = 0.02, 9.21


def case(seed=3, L=70, n=60, K=12):
    """A map with empty slots and correlated covariances, a cloud tight enough that many particles match and loose enough that
    many do not, detections on landmarks and two on nothing, distinct correlated Q_k."""
    rng = np.random.default_rng(seed)
    M = np.zeros((5, L), np.float32)
    M[0], M[1] = rng.uniform(-8, 8, L), rng.uniform(-8, 8, L)
    sx, sy, r = rng.uniform(0.02, 0.3, L), rng.uniform(0.02, 0.3, L), rng.uniform(-0.8, 0.8, L)
    M[2], M[3], M[4] = sx * sx, r * sx * sy, sy * sy
    M[2, rng.random(L) < 0.3] = -1.0
    x, y, th = (0.15 * rng.standard_normal(n)).astype(F), (0.15 * rng.standard_normal(n)).astype(F), (0.02 * rng.standard_normal(n)).astype(F)
    pick = np.flatnonzero(~(M[2] < 0))[:K - 2]
    zx = np.concatenate([M[0, pick] + 0.02 * rng.standard_normal(K - 2), [30.0, -25.0]]).astype(F)
    zy = np.concatenate([M[1, pick] + 0.02 * rng.standard_normal(K - 2), [30.0, 14.0]]).astype(F)
    a, b, rr = rng.uniform(0.05, 0.2, K), rng.uniform(0.05, 0.2, K), rng.uniform(-0.7, 0.7, K)
    covs = ((a * a).astype(F), (rr * a * b).astype(F), (b * b).astype(F))
    return M, x, y, th, zx, zy, covs


def test_q_times_identity_matches_what_the_isotropic_stage_matches(orc):
    M, x, y, th, zx, zy, _ = case()
    K = len(zx)
    iso = (np.full(K, Q, F), np.zeros(K, F), np.full(K, Q, F))
    a0, s0, l0 = S.localise(M, x, y, th, zx, zy, Q, GATE, -3.0)
    a1, s1, l1 = SD.localise(M, x, y, th, zx, zy, iso, GATE, -3.0)
    assert 0 < s0[:, 0].sum() < len(x) * K
    assert np.array_equal(a0, a1) and np.array_equal(s0, s1)
    # The log-likelihoods: NOT the same bits throughout (49 of these 60 are, the particles that matched nothing among them).
    # R_w = H^T (q I) H is q I only up to the rounding of (c q) c + (s q) s, and the general form computes S^-1 as
    # (c / det, -b / det, a / det) where the isotropic one has its own order.  What holds is closeness: both are float32
    # evaluations of one real expression whose inputs differ by a few ulp of q (2^-22 relative), through a determinant whose
    # cancellation amplifies that by no more than (q + P_max)^2 / det_min < 100 on this map: 1e-4 relative is an order above it
    same = bits(l0) == bits(l1)
    print(f"Q_k = q I: {int(same.sum())} of {len(same)} log-likelihoods have the isotropic stage's bits")
    assert not same.all() and same[s0[:, 0] == 0].all()
    assert np.allclose(l0, l1, rtol=1e-4, atol=0.0)


def test_is_the_rows_pair_on_copies_of_the_map(orc):
    M, x, y, th, zx, zy, covs = case(seed=4)
    n, K = len(x), len(zx)
    rows = np.ascontiguousarray(np.broadcast_to(M, (n,) + M.shape))
    want_a, want_s = AD.associate(rows, x, y, th, None, zx, zy, covs, GATE, GATE, 0)
    _, want_ll = AD.update(rows, x, y, th, None, want_a, zx, zy, covs)
    a, s, ll = SD.localise(M, x, y, th, zx, zy, covs, GATE, 0.0)
    assert 0 < s[:, 0].sum() < n * K
    assert np.array_equal(a, want_a) and np.array_equal(s, want_s) and np.array_equal(bits(ll), bits(want_ll))
    assert np.all(a[:, M[2] < 0] == SD.NONE) and np.all(s[:, 1] == 0) and np.all(s.sum(axis=1) == K)


def test_log_clutter_zero_leaves_the_clutter_step_out(orc):
    M, x, y, th, zx, zy, covs = case(seed=5)
    _, s, ll0 = SD.localise(M, x, y, th, zx, zy, covs, GATE, 0.0)
    _, _, llc = SD.localise(M, x, y, th, zx, zy, covs, GATE, -2.5)
    want, _ = W.add(ll0, s, None, 0.0, -2.5, 0.0)
    assert np.array_equal(bits(llc), bits(want)) and (s[:, 2] > 0).all() and not np.array_equal(bits(llc), bits(ll0))
    nothing = s[:, 0] == 0
    if nothing.any():
        assert np.all(bits(ll0[nothing]) == 0)   # +0: nothing was added, not even a zero term
    with pytest.raises(ValueError):
        SD.localise(M, x, y, th, zx, zy, covs, GATE, 0.5)
