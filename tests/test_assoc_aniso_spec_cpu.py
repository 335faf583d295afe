"""The specification of data association under a 2x2 measurement covariance (tests/_assoc_aniso_spec.py) by itself: its cost
against a float64 evaluation by another route, the table's rules, its composition from _aniso_spec.update, and a case in which
no isotropic gate gives its table.  No GPU.

THE COST AGAINST FLOAT64.  The spec forms m = d^T S^-1 d in the WORLD frame, d = w - mu, S = P + R_w.  The reference forms the same
number in the SENSOR frame, in float64: d_s = z - H (mu - t), S_s = H P H^T + Q, m_64 = d_s^T S_s^-1 d_s.  With u = 2^-24,
lambda_min / lambda_max / kappa those of S_s (S has the same eigenvalues), qm = lambda_max(Q):
  - d carries e_d = 4 u (|t| + |mu| + |d|) + 4 (SINCOS_ABS + u) |z|  (the error of w and of w - mu: test_aniso_spec_cpu.py); it moves m
    by at most  D = 2 sqrt(m / lambda_min) e_d + e_d^2 / lambda_min   (|S^-1 d| <= sqrt(m / lambda_min)); what follows acts on
    m' = m + D, the term of the innovation the arithmetic really sees;
  - every entry of R_w carries e_R = 8 (SINCOS_ABS + 2 u) qm (test_aniso_spec_cpu.py), the three sums P + R_w another u lambda_max:
    e_S = u lambda_max + e_R per entry, at most 2 e_S in norm, and delta m = -d^T S^-1 dS S^-1 d <= 2 e_S m' / lambda_min, with
    g = 1 / (1 - 2 e_S / lambda_min) for the higher orders;
  - det = a cc - b b: two products and a difference, (a cc + b^2 + det) u <= ((kappa + 3) / 2 + 1) u of det (a cc <= (lambda_max +
    lambda_min)^2 / 4, b^2 <= a cc); its reciprocal u; the three entries of S^-1 u each.  The first two are common to the
    entries: (kappa + 7) / 2 u m'.  The third is entrywise, and so are the six roundings of t0, t1 and m (four deep):
    5 u sum |d_j| |S^-1_jk| |d_k| <= 5 u |d|^2 / lambda_min <= 5 u kappa m'  (|S^-1| has the norm of S^-1 for a 2x2 matrix; m' >=
    |d|^2 / lambda_max).
  Together   |m - m_64| <= D + (u (5.5 kappa + 3.5) + 2 g e_S / lambda_min) m'.
"""
import numpy as np
import pytest

import _aniso_spec as S
import _assoc_aniso_spec as AA
import _assoc_spec as A
import _f64_pf as F
from _assoc_aniso_bounds import cost64
from test_aniso_spec_cpu import q_matrix

U, SC = F.U, F.SINCOS_ABS
NONE = AA.NONE
REG = sorted({(r, k) for _, r, k in F.GRID})


@pytest.mark.parametrize("ratio", [1.0, 1e2, 1e4])
@pytest.mark.parametrize("q", sorted({q for q, _, _ in F.GRID}))
def test_cost_within_its_bound_of_the_float64_sensor_frame_term(orc, q, ratio):
    """Every (P / q, kappa(P)) regime of the float64 grid, |pose| up to 1e3; each landmark against its own observation (the pair
    the gate is about) and against seven others (far pairs, m up to 1e15)."""
    rng = np.random.default_rng(int(1e9 * q) + int(ratio) + 7)
    cov = q_matrix(q, ratio, rng.uniform(0, np.pi))
    n, lc = 256, 8
    L = lc * len(REG)
    rows, zx, zy, pose = np.empty((n, 5, L), np.float32), np.empty(L, np.float32), np.empty(L, np.float32), None
    for j, (r, k) in enumerate(REG):
        cols = np.arange(j, L, len(REG))
        pose, rows[:, :, cols], zx[cols], zy[cols] = F.regime_frame(rng, n, lc, q, r, k, pose=pose)
    worst = 0.0
    for k0 in range(0, L, 8):                                          # 8 detections at a time: the observations of landmarks k0 .. k0 + 7
        dx, dy = zx[k0:k0 + 8], zy[k0:k0 + 8]
        seen, m = AA.cost_matrix(rows, *pose, None, dx, dy, cov)
        m64, bound = cost64(rows, *pose, dx, dy, cov)
        assert seen.all() and np.all(np.isfinite(m))
        ratio_ = np.abs(m.astype(np.float64) - m64) / bound
        worst = max(worst, float(ratio_.max()))
        own = ratio_[:, np.arange(k0, k0 + 8), np.arange(8)]
        assert own.max() <= 1.0, f"own pairs: {own.max():.3g} x the bound"
    print(f"lambda_max(Q)={q:g} ratio={ratio:g}: max |m - m_64| / bound {worst:.3g}")
    assert worst <= 1.0


def one_particle(L, seen_at, th=0.0):
    """A particle at the origin, heading th; the landmarks of seen_at {l: (x, y)} seen with P = 1e-6 I, the others not."""
    rows = np.zeros((1, 5, L), np.float32)
    rows[:, 2] = -1.0
    for l, (px, py) in seen_at.items():
        rows[0, :, l] = (px, py, 1e-6, 0.0, 1e-6)
    z = np.zeros(1, np.float32)
    return rows, z, z.copy(), np.full(1, th, np.float32)


COV = (0.02, 0.012, 0.015)
GATE, NEW_GATE = 9.21, 50.0


def tab(rows, x, y, th, zx, zy, cov=COV, gate=GATE, new_gate=NEW_GATE, create=1, **kw):
    return AA.associate(rows, x, y, th, None, np.asarray(zx, np.float32), np.asarray(zy, np.float32), cov, gate, new_gate, create, **kw)


def test_one_to_one_and_ties_to_the_lowest_index(orc):
    # two bit-identical landmarks and one detection on them: the lower landmark takes it, the other gets nothing
    rows, x, y, th = one_particle(6, {1: (3.0, 1.0), 4: (3.0, 1.0), 2: (-2.0, 0.5)})
    assoc, st = tab(rows, x, y, th, [3.0, -2.0], [1.0, 0.5])
    assert assoc[0].tolist() == [NONE, 0, 1, NONE, NONE, NONE] and st[0].tolist() == [2, 0, 0]
    # two bit-identical detections on one landmark: the landmark takes the lower one; the other is near it, so it starts nothing
    assoc, st = tab(rows, x, y, th, [9.0, -2.0, -2.0], [9.0, 0.5, 0.5])
    assert assoc[0].tolist() == [0, NONE, 1, NONE, NONE, NONE] and st[0].tolist() == [1, 1, 1]
    # two landmarks that choose the same detection: the cheaper one gets it, the other gets nothing although a second detection
    # lies inside its gate (a landmark asks for its cheapest detection only)
    rows, x, y, th = one_particle(3, {0: (1.0, 0.0), 1: (1.2, 0.0)})
    assoc, st = tab(rows, x, y, th, [1.08, 1.35], [0.0, 0.0])
    seen, m = AA.cost_matrix(rows, x, y, th, None, np.array([1.08, 1.35], np.float32), np.zeros(2, np.float32), COV)
    assert m[0, 0, 0] < m[0, 1, 0] < m[0, 1, 1] <= GATE               # both prefer detection 0, landmark 0 is nearer to it
    assert assoc[0].tolist() == [0, NONE, NONE] and st[0].tolist() == [1, 0, 1]
    # every table: no detection twice
    for row in assoc:
        ks = row[row != NONE]
        assert len(np.unique(ks)) == len(ks)


def test_nan_priors_are_never_candidates_and_never_near(orc):
    rows, x, y, th = one_particle(4, {0: (2.0, 0.0), 1: (5.0, 5.0)})
    rows[0, 3, 0] = np.nan                                              # seen (P_xx >= 0), but every cost is NaN
    assoc, st = tab(rows, x, y, th, [2.0], [0.0])
    assert assoc[0].tolist() == [NONE, NONE, 0, NONE] and st[0].tolist() == [0, 1, 0]   # not matched, not "near": a new landmark
    rows[0, 2, 1] = np.nan                                              # NaN P_xx: not "< 0", so seen, and again no candidate
    assoc, st = tab(rows, x, y, th, [5.0], [5.0])
    assert assoc[0].tolist() == [NONE, NONE, 0, NONE]


def test_creation_order_running_out_of_slots_create_0_and_no_detections(orc):
    rows, x, y, th = one_particle(5, {1: (1.0, 1.0), 3: (-4.0, 2.0)})
    zx, zy = [7.0, 1.0, -7.0, 6.0, 0.0], [7.0, 1.0, 7.0, -6.0, -8.0]    # detection 1 is landmark 1; the other four are new
    assoc, st = tab(rows, x, y, th, zx, zy)
    assert assoc[0].tolist() == [0, 1, 2, NONE, 3] and st[0].tolist() == [1, 3, 1]   # ascending k into ascending unseen l, one dropped
    assoc, st = tab(rows, x, y, th, zx, zy, create=0)
    assert assoc[0].tolist() == [NONE, 1, NONE, NONE, NONE] and st[0].tolist() == [1, 0, 4]
    assoc, st = tab(rows, x, y, th, zx, zy, assoc_stride=8)
    assert assoc.shape == (1, 8) and np.all(assoc[0, 5:] == NONE)       # the padding
    assoc, st = tab(rows, x, y, th, [], [])
    assert np.all(assoc == NONE) and st[0].tolist() == [0, 0, 0]
    out, ll = AA.update(rows, x, y, th, None, assoc, np.zeros(0, np.float32), np.zeros(0, np.float32), COV)
    assert np.array_equal(out.view(np.uint32), rows.view(np.uint32)) and ll[0] == 0


def test_the_update_is_aniso_spec_update_particle_by_particle(orc):
    """... with the table's list, out of place through a gather index and in place; a created landmark holds the world_noise of
    the particle that created it, bit for bit."""
    from test_gpu_aniso import make_case                                 # (a helper without a GPU in it)
    from test_gpu_assoc import detections
    n, L, Lp = 40, 70, 96
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 5)
    dx, dy = detections(zx, zy, 50, 2)
    anc = np.random.default_rng(1).integers(0, n, n).astype(np.int32)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    for cov in (COV, (4e-6, 0.0, 4e-2)):
        for a in (None, anc):
            assoc, st = AA.associate(rows, x, y, th, a, dx, dy, cov, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
            assert st[:, 0].sum() > 0 and st[:, 1].sum() > 0
            got, got_ll = AA.update(rows, x, y, th, a, assoc, dx, dy, cov, L=L, in_place=False)
            src = np.arange(n) if a is None else a
            for i in range(n):
                ids = np.flatnonzero(assoc[i, :L] != NONE)
                k = assoc[i, ids].astype(np.int64)
                want, want_ll = S.update(rows[src[i]:src[i] + 1], x[i:i + 1], y[i:i + 1], th[i:i + 1], None, ids, dx[k], dy[k], cov, L=L)
                assert np.array_equal(bits(got[i, :, :L]), bits(want[0, :, :L])) and bits(got_ll[i:i + 1]) == bits(want_ll), (i, a is None)
            # created: the slot was unseen in the source row and took a detection
            created = (rows[src][:, 2, :L] < 0) & (assoc[:, :L] != NONE)
            assert created.any()
            s, c = orc.det_sincos(th)
            rw = S.world_noise(cov, s, c)
            for j in range(3):
                assert np.array_equal(bits(got[:, 2 + j, :L][created]), bits(np.broadcast_to(rw[j][:, None], (n, L))[created]))
        assoc, _ = AA.associate(rows, x, y, th, None, dx, dy, cov, GATE, NEW_GATE, 1, L=L)
        same, same_ll = AA.update(rows, x, y, th, None, assoc, dx, dy, cov, L=L, in_place=True)
        out, out_ll = AA.update(rows, x, y, th, None, assoc, dx, dy, cov, L=L)
        assert np.array_equal(bits(same), bits(out)) and np.array_equal(bits(same_ll), bits(out_ll))


def test_no_isotropic_gate_gives_this_table(orc):
    """One particle at the origin looking along x, one landmark 5 m ahead with a small prior (1e-6 I), Q = diag(4e-6, 4e-2): 2 mm
    along the beam, 20 cm across.  Detection 0 lies 30 cm ACROSS the beam from the landmark (1.5 sigma: the landmark), detection 1
    lies 5 cm ALONG it (22 sigma: something else).
      under R_w:              the landmark takes detection 0, detection 1 starts a new landmark;
      meas_var = 4e-2 (large): detection 1 is the cheaper of two candidates and wins, detection 0 is near and is dropped;
      meas_var = 4e-6 (small): neither is within new_gate of the landmark: two new landmarks beside it.
    The new stage is not the old one with another scalar."""
    q = (4e-6, 0.0, 4e-2)
    rows, x, y, th = one_particle(3, {0: (5.0, 0.0)})
    zx, zy = np.array([5.0, 5.05], np.float32), np.array([0.3, 0.0], np.float32)
    seen, m = AA.cost_matrix(rows, x, y, th, None, zx, zy, q)
    assert m[0, 0, 0] < GATE and m[0, 0, 1] > NEW_GATE
    assoc, st = AA.associate(rows, x, y, th, None, zx, zy, q, GATE, NEW_GATE, 1)
    assert assoc[0].tolist() == [0, 1, NONE] and st[0].tolist() == [1, 1, 0]
    large, st_l = A.associate(rows, x, y, th, None, zx, zy, 4e-2, GATE, NEW_GATE, 1)
    assert large[0].tolist() == [1, NONE, NONE] and st_l[0].tolist() == [1, 0, 1]
    small, st_s = A.associate(rows, x, y, th, None, zx, zy, 4e-6, GATE, NEW_GATE, 1)
    assert small[0].tolist() == [NONE, 0, 1] and st_s[0].tolist() == [0, 2, 0]
    # turned by a quarter (w = t + H^T z puts the point 5 m ahead at (0, -5)): R_w turns with the heading, the table does not change
    rows90, x, y, th90 = one_particle(3, {0: (0.0, -5.0)}, th=np.pi / 2)
    assoc90, _ = AA.associate(rows90, x, y, th90, None, zx, zy, q, GATE, NEW_GATE, 1)
    assert assoc90[0].tolist() == [0, 1, NONE]
