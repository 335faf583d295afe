"""The specification of data association under a measurement covariance per detection (tests/_assoc_detcov_spec.py) by itself:
what it equals when every Q_k is the same, its composition from _aniso_spec.update, a case whose table no single Q gives, and its
update against an independent float64 sensor-frame EKF.  No GPU.

THE UPDATE AGAINST FLOAT64.  Landmark l of particle i is updated with R_w(i, k), k = assoc[i][l], and det Q_k: for that pair the
arithmetic is _aniso_spec.update_one's, operation for operation, with Q_k where that test has Q.  The forward-error bounds of
tests/test_aniso_spec_cpu.py (its docstring holds the derivation) therefore hold PAIR BY PAIR with each pair's own quantities —
qm = lambda_max(Q_k), e_R = 8 (SINCOS_ABS + 2 u) qm for the rounding of that pair's R_w, S = P + R_w(i, k), kappa(S), lambda_min(S),
a_P = max(1, ||P S^-1||_2) of that S, and the rounding of det Q_k = qxx qyy - qxy^2 (4 u (qxx qyy + qxy^2) lambda_max(P) / det S,
the term that test already carries: there it is rounded once per session, here once per pair, by the same three operations) — and
nothing is added: no value is shared between pairs except the pose and (s, c), whose errors the bounds already charge to every
pair.  The reference is test_aniso_spec_cpu.ekf64 (H = [[c, -s], [s, c]], S = H P H^T + Q_k, K = P H^T S^-1, mu' = mu + K nu,
P' = (I - K H) P), called once per detection with that detection's Q_k on the columns that take it.  The particle's
log-likelihood: the sum of its pairs' bounds plus the (ceil(L / 128) + 7) u sum |ll| of the summation tree, as there.
"""
import numpy as np
import pytest

import _aniso_spec as S
import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _assoc_spec as A
import _f64_pf as F
from _aniso_bounds import check_pairs, q_matrix

U, SC = F.U, F.SINCOS_ABS
NONE = AD.NONE
GATE, NEW_GATE = 9.21, 50.0
bits = lambda a: np.ascontiguousarray(a).view(np.uint32)


def case(n=40, L=70, Lp=96, K=50, seed=5):
    from test_gpu_aniso import make_case                                 # (helpers without a GPU in them)
    from test_gpu_assoc import detections
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, seed)
    dx, dy = detections(zx, zy, K, 2)
    anc = np.random.default_rng(1).integers(0, n, n).astype(np.int32)
    return x, y, th, rows, dx, dy, anc


def different_covs(K, seed, qm=0.04):
    rng = np.random.default_rng(seed)
    q = np.array([q_matrix(qm * 10.0 ** rng.uniform(-1, 0), 10.0 ** rng.uniform(0, 4), rng.uniform(0, np.pi)) for _ in range(K)], np.float32)
    return q[:, 0].copy(), q[:, 1].copy(), q[:, 2].copy()


def test_every_q_k_equal_is_the_aniso_spec_and_q_i_the_isotropic_tables(orc):
    n, L, Lp, K = 40, 70, 96, 50
    x, y, th, rows, dx, dy, anc = case(n, L, Lp, K)
    for cov in ((0.02, 0.012, 0.015), (4e-6, 0.0, 4e-2)):
        covs = tuple(np.full(K, v, np.float32) for v in cov)
        for a in (None, anc):
            for create in (0, 1):
                got, got_st = AD.associate(rows, x, y, th, a, dx, dy, covs, GATE, NEW_GATE, create, L=L, assoc_stride=Lp)
                want, want_st = AA.associate(rows, x, y, th, a, dx, dy, cov, GATE, NEW_GATE, create, L=L, assoc_stride=Lp)
                assert np.array_equal(got, want) and np.array_equal(got_st, want_st)
            assert want_st[:, 0].sum() > 0 and want_st[:, 1].sum() > 0
            out, ll = AD.update(rows, x, y, th, a, want, dx, dy, covs, L=L)
            ref, ref_ll = AA.update(rows, x, y, th, a, want, dx, dy, cov, L=L)
            assert np.array_equal(bits(out), bits(ref)) and np.array_equal(bits(ll), bits(ref_ll))
        seen, m = AD.cost_matrix(rows, x, y, th, None, dx, dy, covs, L=L)
        seen_a, m_a = AA.cost_matrix(rows, x, y, th, None, dx, dy, cov, L=L)
        assert np.array_equal(seen, seen_a) and np.array_equal(bits(m), bits(m_a))
    q = np.float32(0.02)
    covs = (np.full(K, q), np.zeros(K, np.float32), np.full(K, q))
    for a in (None, anc):
        got, got_st = AD.associate(rows, x, y, th, a, dx, dy, covs, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        want, want_st = A.associate(rows, x, y, th, a, dx, dy, q, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        assert np.array_equal(got, want) and np.array_equal(got_st, want_st)


def test_the_update_is_aniso_spec_update_once_per_distinct_detection(orc):
    """Particle by particle: _aniso_spec.update called once per distinct k the particle's table names, with that detection's Q_k
    and the landmarks that take it, gives the row; the particle's terms go through the one summation.  A created landmark holds
    world_noise(Q_k) of the detection that made it."""
    n, L, Lp, K = 40, 70, 96, 50
    x, y, th, rows, dx, dy, anc = case(n, L, Lp, K)
    covs = different_covs(K, 3)
    s, c = orc.det_sincos(th)
    for a in (None, anc):
        assoc, st = AD.associate(rows, x, y, th, a, dx, dy, covs, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        assert st[:, 0].sum() > 0 and st[:, 1].sum() > 0
        got, got_ll = AD.update(rows, x, y, th, a, assoc, dx, dy, covs, L=L)
        src = np.arange(n) if a is None else a
        for i in range(n):
            row = rows[src[i]:src[i] + 1]
            want = row.copy()
            terms = np.zeros((1, L), np.float32)
            for k in np.unique(assoc[i, :L][assoc[i, :L] != NONE]):
                ids = np.flatnonzero(assoc[i, :L] == k)
                q_k = (covs[0][k], covs[1][k], covs[2][k])
                one, _ = S.update(row, x[i:i + 1], y[i:i + 1], th[i:i + 1], None, ids, np.full(len(ids), dx[k]), np.full(len(ids), dy[k]), q_k, L=L)
                want[0][:, ids] = one[0][:, ids]
                # the landmark's term, from the same call on that landmark alone: a sum of one term is that term (+0 elsewhere)
                for l in ids:
                    _, t = S.update(row, x[i:i + 1], y[i:i + 1], th[i:i + 1], None, [l], dx[k:k + 1], dy[k:k + 1], q_k, L=L)
                    terms[0, l] = t[0]
            assert np.array_equal(bits(got[i, :, :L]), bits(want[0, :, :L])), (i, a is None)
            assert bits(got_ll[i:i + 1]) == bits(S.sum_loglik(terms)), (i, a is None)
        created = (rows[src][:, 2, :L] < 0) & (assoc[:, :L] != NONE)
        assert created.any()
        ii, ll_ = np.nonzero(created)
        k = assoc[ii, ll_].astype(np.int64)
        rw = S.world_noise((covs[0][k], covs[1][k], covs[2][k]), s[ii], c[ii])
        for j in range(3):
            assert np.array_equal(bits(got[ii, 2 + j, ll_]), bits(rw[j]))
    assoc, _ = AD.associate(rows, x, y, th, None, dx, dy, covs, GATE, NEW_GATE, 1, L=L)
    same, same_ll = AD.update(rows, x, y, th, None, assoc, dx, dy, covs, L=L, in_place=True)
    out, out_ll = AD.update(rows, x, y, th, None, assoc, dx, dy, covs, L=L)
    assert np.array_equal(bits(same), bits(out)) and np.array_equal(bits(same_ll), bits(out_ll))


def test_no_single_q_gives_this_table(orc):
    """One particle at the origin looking along x.  Pole A is dead ahead at (5, 0), pole B abeam at (0, 5); each is seen with
    noise tight along its own beam (2 mm) and loose across it (20 cm): Q_A = diag(4e-6, 4e-2), Q_B = diag(4e-2, 4e-6).  Each pole
    has a neighbour 5 cm away ALONG its beam — across its tight axis, 25 sigma: another object — and is itself detected 30 cm
    ACROSS its beam (1.5 sigma: the pole).  Detections: 0 = A displaced across, 1 = A's neighbour, 2 = B displaced across,
    3 = B's neighbour; landmarks 0 = A, 1 = B.
      per detection: A takes 0, B takes 2, the neighbours start landmarks 2 and 3;
      everything under Q_A: right for A; B's beam runs along y, where Q_A is loose: detection 3 (5 cm along y) is the cheaper of
                            B's candidates and wins, detection 2 (30 cm along x, 150 sigma) is far and starts a landmark;
      everything under Q_B: the mirror image: A takes its neighbour's detection."""
    q_a, q_b = (4e-6, 0.0, 4e-2), (4e-2, 0.0, 4e-6)
    rows = np.zeros((1, 5, 5), np.float32)
    rows[:, 2] = -1.0
    rows[0, :, 0] = (5.0, 0.0, 1e-6, 0.0, 1e-6)
    rows[0, :, 1] = (0.0, 5.0, 1e-6, 0.0, 1e-6)
    z = np.zeros(1, np.float32)
    zx, zy = np.array([5.0, 5.05, 0.3, 0.0], np.float32), np.array([0.3, 0.0, 5.0, 5.05], np.float32)
    per_det = tuple(np.array([q_a[j], q_a[j], q_b[j], q_b[j]], np.float32) for j in range(3))
    seen, m = AD.cost_matrix(rows, z, z, z, None, zx, zy, per_det)
    assert m[0, 0, 0] < GATE and m[0, 0, 1] > NEW_GATE and m[0, 1, 2] < GATE and m[0, 1, 3] > NEW_GATE
    assoc, st = AD.associate(rows, z, z, z, None, zx, zy, per_det, GATE, NEW_GATE, 1)
    assert assoc[0].tolist() == [0, 2, 1, 3, NONE] and st[0].tolist() == [2, 2, 0]
    tables = {}
    for name, q in (("Q_A", q_a), ("Q_B", q_b)):
        single = tuple(np.full(4, v, np.float32) for v in q)
        tables[name], _ = AD.associate(rows, z, z, z, None, zx, zy, single, GATE, NEW_GATE, 1)
        ref, _ = AA.associate(rows, z, z, z, None, zx, zy, q, GATE, NEW_GATE, 1)
        assert np.array_equal(tables[name], ref)
    assert tables["Q_A"][0].tolist() == [0, 3, 1, 2, NONE]              # B took its neighbour's detection
    assert tables["Q_B"][0].tolist() == [1, 2, 0, 3, NONE]              # A took its neighbour's detection
    assert len({tuple(t[0]) for t in tables.values()} | {tuple(assoc[0])}) == 3
    # turned by a quarter, the poles where that heading sees them at the same sensor-frame points: nothing changes
    rows90 = rows.copy()
    rows90[0, :2, 0] = (0.0, -5.0)                                      # w = t + H^T z: (5, 0) ahead lies at (0, -5)
    rows90[0, :2, 1] = (5.0, 0.0)
    th90 = np.full(1, np.pi / 2, np.float32)
    assoc90, _ = AD.associate(rows90, z, z, th90, None, zx, zy, per_det, GATE, NEW_GATE, 1)
    assert assoc90[0].tolist() == assoc[0].tolist()


N, LC = 4096, 5
REG = sorted({(r, k) for _, r, k in F.GRID})
RATIOS = (1.0, 1e1, 1e2, 1e3, 1e4)


@pytest.mark.parametrize("q", sorted({q for q, _, _ in F.GRID}))
def test_update_within_its_bounds_of_the_float64_ekf(orc, q):
    """n = 4096, L = 75 (landmark l in regime l mod 15 of the float64 grid at this q: P / q from 1e-4 to 1e8, kappa(P) up to 1e4 —
    near-singular priors —, |pose| up to 1e3 m, 10 % first sightings), K = 64: detection k is the observation of landmark perm[k],
    11 landmarks take none; Q_k has lambda_max = q, a : b from 1 : 1 to 1 : 1e4 (k mod 5) and its own axis."""
    rng = np.random.default_rng(int(1e9 * q) + 11)
    L, K = LC * len(REG), 64
    rows, zx, zy, pose = np.empty((N, 5, L), np.float32), np.empty(L, np.float32), np.empty(L, np.float32), None
    for j, (r, k) in enumerate(REG):
        cols = np.arange(j, L, len(REG))
        pose, rows[:, :, cols], zx[cols], zy[cols] = F.regime_frame(rng, N, LC, q, r, k, pose=pose)
    rows[:, 2][rng.random((N, L)) < 0.1] = -1.0
    x, y, th = pose
    assert np.hypot(x, y).max() >= 100.0
    perm = rng.permutation(L)[:K]
    dx, dy = zx[perm], zy[perm]
    cov = [q_matrix(q, RATIOS[k % 5], rng.uniform(0, np.pi)) for k in range(K)]
    covs = tuple(np.array([c[j] for c in cov], np.float32) for j in range(3))
    assert AD.valid_covs(covs)
    assoc = np.full((N, L), NONE, np.uint8)
    assoc[:, perm] = np.arange(K, dtype=np.uint8)[None, :]
    out, ll = AD.update(rows, x, y, th, None, assoc, dx, dy, covs)
    untouched = np.setdiff1d(np.arange(L), perm)
    assert np.array_equal(bits(out[:, :, untouched]), bits(rows[:, :, untouched]))
    check_pairs(rows, out, ll, (x, y, th), perm, dx, dy, cov, f"lambda_max(Q)={q:g}")
