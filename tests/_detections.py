"""Generators of a frame's detections and of their per-detection covariances.  TEST INFRASTRUCTURE shared by the association
tests (test_gpu_assoc*.py), the CPU specification tests and the regime populations (tests/_regimes.py); numpy only."""
import numpy as np

import _assoc_detcov_spec as AD
from _aniso_bounds import q_matrix


def detections(zx, zy, K, seed):
    """K detections: observations of landmarks of the case in shuffled order (their identity is what the kernel has to find), and
    once those run out points that belong to nothing."""
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(zx))[:K]
    dx = np.concatenate([zx[pick], rng.uniform(-20, 20, K - len(pick)).astype(np.float32)])
    dy = np.concatenate([zy[pick], rng.uniform(-20, 20, K - len(pick)).astype(np.float32)])
    return dx.astype(np.float32), dy.astype(np.float32)


def covariances(K, seed, qm=0.04):
    """Every Q_k different: the large eigenvalue within a decade of qm, a : b from 1 : 1 to 1 : 1e4, the axes turned per detection."""
    rng = np.random.default_rng(seed)
    q = [q_matrix(qm * 10.0 ** rng.uniform(-1, 0), 10.0 ** rng.uniform(0, 4), rng.uniform(0, np.pi)) for _ in range(K)]
    q = np.array(q, np.float32).reshape(K, 3)
    assert AD.valid_covs(q.T)
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()
