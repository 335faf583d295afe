"""tests/_spread_spec.py — the exact restatement of slam_pf_spread that tests/test_gpu_spread.py holds the kernels to — against
float64 math with a DERIVED bound, and the properties a covariance has to have.  Needs no GPU."""
import numpy as np
import pytest

import _estimate_spec as E
import _spread_spec as S
from conftest import bits

DET_SINCOS_ERR = 2.5e-7          # |det_sincos - libm| on [-20, 20]: tests/test_oracle_pf.py::test_det_math_accuracy
SIZES = [1, 2, 63, 64, 65, 257, 2049]


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _bound(dmax, k, cov_k):
    """The bound on |cov[k] - float64 covariance about the same mean|, written out.  A delta a_i goes in as A_i * 2^-20 with
    |A_i * 2^-20 - a_i| < e_a: less than one unit of 2^-20 for the truncation, half an ulp of the binary32 subtraction, and for the
    sine the stated error of det_sincos.  So every product is off by less than e_a max|b| + e_b max|a| + e_a e_b — the quantisation,
    2 * 2^-20 * max|d| when both are lengths — and so is their (weighted) mean; the truncated quotient loses less than one unit of
    2^-40; half an ulp for the final binary32 rounding; 2^-48 relative for the float64 arithmetic on either side."""
    e = [2.0 ** -20 + 0.5 * _ulp32(dmax[0]), 2.0 ** -20 + 0.5 * _ulp32(dmax[1]), 2.0 ** -20 + DET_SINCOS_ERR + 0.5 * _ulp32(dmax[3])]
    i, j = S.PAIRS[k]
    return (e[i] * dmax[j] + e[j] * dmax[i] + e[i] * e[j] + 2.0 ** -40 + 0.5 * _ulp32(cov_k) + 2.0 ** -48 * dmax[i] * dmax[j])


POPULATIONS = [("plain", E.edge_population), ("negative", E.edge_population), ("two_clusters", S.spread_population),
               ("far_cloud", S.spread_population), ("off_grid", S.spread_population)]


@pytest.mark.parametrize("name,make", POPULATIONS)
@pytest.mark.parametrize("n", SIZES)
def test_spread_spec_against_float64(orc, name, make, n):
    x, y, th = make(name, n)
    rng = np.random.default_rng(n)
    idx = np.sort(rng.integers(0, n, n)).astype(np.int32)          # a pending gather: repeats and gaps
    w16 = [int(v) for v in rng.integers(0, 2 ** 16 + 1, n)]
    w16[0] = 2 ** 16
    for ref in (0.0, 0.6):
        for gather in (None, idx):
            for w in (None, w16):
                pose, cov, r, (sums, d) = S.spread_spec(x, y, th, gather, ref, n, w)
                assert np.array_equal(bits(pose), bits(E.mean_spec(x, y, th, gather, ref, n, w)[0]))
                assert d == (n if w is None else sum(w))
                g = slice(None) if gather is None else gather
                want = S.f64_cov(x[g], y[g], th[g], pose, w)
                dth = th[g].astype(np.float64) - float(pose[2])
                dmax = [float(np.abs(x[g].astype(np.float64) - float(pose[0])).max()),
                        float(np.abs(y[g].astype(np.float64) - float(pose[1])).max()), 1.0, float(np.abs(dth).max())]
                for k in range(6):
                    assert abs(float(cov[k]) - want[k]) <= _bound(dmax, k, cov[k]), (name, n, ref, k, float(cov[k]), want[k])
                _, _, _, rr = E.f64_means(x[g], y[g], th[g], ref, w)
                # heading_r: a term sin / cos(th_i - ref) is off by the stated error of det_sincos, one unit of 2^-30 and half an ulp of
                # the binary32 difference; the mean vector moves by at most sqrt(2) times that plus a unit of 2^-30 per component for
                # the truncated quotients, and its length by no more; half an ulp of 1 for the final rounding
                dref = float(np.abs(th[g].astype(np.float64) - float(np.float32(ref))).max())
                br = 2.0 ** 0.5 * (DET_SINCOS_ERR + 2.0 ** -29 + 0.5 * _ulp32(dref)) + 0.5 * _ulp32(1.0)
                assert abs(float(r) - rr) <= br, (name, n, float(r), rr, br)


@pytest.mark.parametrize("n", [65, 2049])
def test_truncation_and_floor_are_told_apart(orc, n):
    """off_grid: most deltas are negative and none sits on the 2^-20 grid, so a kernel that floors gives other sums in every entry."""
    x, y, th = S.spread_population("off_grid", n)
    pose, _, _, (trunc_sums, _) = S.spread_spec(x, y, th, None, 0.0, n)
    dx, dy, ss = S.deltas(x, y, th, None, pose)
    assert sum(v < 0 for v in dx) > n // 2 and sum(v < 0 for v in dy) > n // 2 and sum(v < 0 for v in ss) > n // 2
    assert S.deltas(x, y, th, None, pose, E.floor_fixed) != (dx, dy, ss)
    floor_sums = S.moment_sums(x, y, th, None, pose, None, E.floor_fixed)[0]
    assert all(a != b for a, b in zip(trunc_sums, floor_sums)), (trunc_sums, floor_sums)
    assert not np.array_equal(bits(S.cov_from_sums(trunc_sums, n)), bits(S.cov_from_sums(floor_sums, n)))


@pytest.mark.parametrize("n", [1, 2, 65, 2049])
def test_identical_poses_give_exact_zeros(orc, n):
    """... +0 in all six entries (also where the mean is not the pose itself: y = -1e-7 has bits under 2^-32), and one heading."""
    for pop in (S.spread_population("identical", n), tuple(a[:1].repeat(n) for a in E.edge_population("negative", 4))):
        for w in (None, [3] * n):
            pose, cov, r, _ = S.spread_spec(*pop, None, 2.9, n, w)
            assert not np.any(bits(cov)), cov.tolist()
            assert abs(float(r) - 1.0) <= 2.0 ** 0.5 * (DET_SINCOS_ERR + 2.0 ** -29) + 0.5 * _ulp32(1.0)   # (sin^2 + cos^2 of det_sincos)


def test_translation_leaves_the_covariance_alone(orc):
    """Deltas that are exactly representable before and after: a population symmetric about 0 on the 2^-10 grid, moved by
    (512, -256) — same bits."""
    n = 128
    rng = np.random.default_rng(5)
    half = rng.integers(-4096, 4097, (2, n // 2)).astype(np.float32) * np.float32(2.0 ** -10)
    x, y = (np.concatenate([h, -h]) for h in half)
    th = rng.normal(0.0, 0.3, n).astype(np.float32)
    pose, cov, r, (sums, _) = S.spread_spec(x, y, th, None, 0.0, n)
    assert pose[0] == 0 and pose[1] == 0 and cov[0] > 0.5
    moved = S.spread_spec(x + np.float32(512.0), y - np.float32(256.0), th, None, 0.0, n)
    assert moved[0][0] == 512.0 and moved[0][1] == -256.0 and moved[3][0] == sums
    assert np.array_equal(bits(moved[1]), bits(cov)) and np.array_equal(bits(moved[2]), bits(r))


@pytest.mark.parametrize("name,make", POPULATIONS)
def test_symmetric_positive_semidefinite(orc, name, make):
    """Cauchy-Schwarz holds for the exact sums; the truncated quotients keep it up to one unit each: (q0 + 1)(q2 + 1) >= q1^2, and
    likewise for the other two pairs of axes."""
    n = 257
    x, y, th = make(name, n)
    w16 = [int(v) for v in np.random.default_rng(1).integers(1, 2 ** 16 + 1, n)]
    for w in (None, w16):
        _, cov, _, (sums, d) = S.spread_spec(x, y, th, None, 0.1, n, w)
        q = [E.trunc_div(t, d) for t in sums]
        for a, b, ab in ((0, 2, 1), (0, 5, 3), (2, 5, 4)):
            assert sums[a] >= 0 and sums[b] >= 0 and sums[a] * sums[b] >= sums[ab] ** 2
            assert (q[a] + 1) * (q[b] + 1) >= q[ab] ** 2, (name, a, b)
            assert cov[a] >= 0 and cov[b] >= 0


def test_out_of_domain_is_refused(orc):
    n = 65537
    S.spread_spec(*S.boundary_population(n, 2047.9), None, 0.3, n)
    with pytest.raises(S.OutOfDomain):
        S.spread_spec(*S.boundary_population(n, 2048.1), None, 0.3, n)
    nan = list(S.boundary_population(65, 1.0))
    nan[1][3] = np.nan
    with pytest.raises(S.OutOfDomain):
        S.deltas(*nan, None, (1.0, -2.0, 0.3))


@pytest.mark.parametrize("shards", [2, 3, 8])
def test_shards_add_to_the_whole(orc, shards):
    """The sums of a population split into shards (about the mean of the whole) add to the unsplit sums, weights and all."""
    n = 2049 - 2049 % shards
    x, y, th = E.edge_population("plain", n)
    w16 = [int(v) for v in np.random.default_rng(2).integers(0, 2 ** 16 + 1, n)]
    for w in (None, w16):
        pose, _, _, (sums, d) = S.spread_spec(x, y, th, None, 0.07, n, w)
        m = n // shards
        parts = [S.moment_sums(x[r * m:(r + 1) * m], y[r * m:(r + 1) * m], th[r * m:(r + 1) * m], None, pose,
                               None if w is None else w[r * m:(r + 1) * m]) for r in range(shards)]
        assert [sum(p[0][k] for p in parts) for k in range(6)] == sums
        assert sum(p[1] for p in parts) == d
