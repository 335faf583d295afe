"""slam_localise_detcov_dev (localisation in a known map under a covariance per detection, csrc/localise_kernels.hip) against the
specification tests/_localise_detcov_spec.py: the table's bytes, the stats and the log-likelihood's bits are equal exactly — whatever
the shape, with unseen slots scattered through the map, ties between landmarks and between detections that carry the same Q, a
detection outside every gate and one exactly on it, a NaN pose, with and without a table pointer, on the staged and on the
unstaged path.  The shapes are those of test_gpu_localise.py."""
import numpy as np
import pytest
import torch

import _assoc_detcov_spec as AD
import _localise_detcov_spec as S
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_localise import DEV, GATE, dev, host, make_detections, make_map, make_poses

pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for torch's fills and copies and the engine's launches
    yield e
    torch.cuda.synchronize()
    e.close()


def covariances(K, seed):
    """K distinct positive definite Q_k: standard deviations of 5 to 25 cm, each with a correlation."""
    rng = np.random.default_rng(seed)
    a, b, r = rng.uniform(0.05, 0.25, K), rng.uniform(0.05, 0.25, K), rng.uniform(-0.8, 0.8, K)
    return (a * a).astype(F), (r * a * b).astype(F), (b * b).astype(F)


def raw_map(M, Lp):
    raw = np.zeros((5, Lp), np.float32)
    raw[2] = -1.0
    raw[:, :M.shape[1]] = M
    return dev(raw)


def run(eng, d_map, Lp, L, x, y, th, zx, zy, covs, gate=GATE, table=True, stride=None):
    n = len(x)
    stride = L if stride is None else stride
    d_assoc = torch.full((n, stride), 7, dtype=torch.uint8, device=DEV) if table else None
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    d_ll = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
    eng.detections_upload(zx, zy)
    eng.detections_cov_upload(*covs)
    eng.localise_detcov_dev(d_map, Lp, L, dev(x), dev(y), dev(th), n, gate, d_assoc, stride, d_st, d_ll)
    return (host(d_assoc) if table else None), host(d_st), host(d_ll)


def check(eng, M, x, y, th, zx, zy, covs, gate=GATE, stride=None, label=""):
    """One launch against the spec: table (the whole stride), stats, ll bits; then the same without a table pointer."""
    L = M.shape[1]
    Lp = (L + 31) // 32 * 32
    stride = L if stride is None else stride
    want, want_st, want_ll = S.localise(M, x, y, th, zx, zy, covs, gate, 0.0)
    want = np.concatenate([want, np.full((len(x), stride - L), S.NONE, np.uint8)], axis=1)
    d_map = raw_map(M, Lp)
    got, got_st, got_ll = run(eng, d_map, Lp, L, x, y, th, zx, zy, covs, gate, True, stride)
    assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: ll differs at {np.flatnonzero(bits(got_ll) != bits(want_ll))[:5].tolist()}"
    _, st2, ll2 = run(eng, d_map, Lp, L, x, y, th, zx, zy, covs, gate, False)
    assert np.array_equal(st2, want_st) and np.array_equal(bits(ll2), bits(want_ll)), f"{label}: without a table pointer"
    return want, want_st, want_ll


@pytest.mark.parametrize("K", (0, 1, 17, 64))
@pytest.mark.parametrize("L", (1, 64, 129, 200))
def test_equals_the_spec(eng, L, K):
    """n = 130: a last workgroup with 2 of 4 wavefronts; a stride with padding columns, every other case one that is no multiple of
    4 (the byte path of the write-out)."""
    n = 130
    M = make_map(L, 100 + L)
    true, x, y, th = make_poses(n, L + K)
    zx, zy = make_detections(M, true, K, 7 * L + K)
    _, st, ll = check(eng, M, x, y, th, zx, zy, covariances(K, 11 * L + K), stride=(L + 35) // 32 * 32 if K % 2 == 0 else L + 3,
                      label=f"L={L} K={K}")
    assert np.all(st[:, 1] == 0) and np.all(st.sum(axis=1) == K)
    if K == 0:
        assert np.all(bits(ll) == 0)   # +0
    if K >= 17 and L >= 64:
        assert 0 < st[:, 0].sum() < n * K   # (the case exercises both outcomes)


def tie_case():
    """-> (M, x, y, th, zx, zy, covs, gate_on): test_gpu_localise.tie_case under distinct Q_k — landmarks 150 and 70 are bit-identical
    copies of 5 and 66, detection 7 of detection 2 AND OF ITS Q; detection 19 lies outside every gate; particle 11 has x = NaN;
    gate_on is the cost of (particle 20, landmark 66, detection 1) by the spec's own operations."""
    n, L = 130, 200
    M = make_map(L, 5)
    M[2, [5, 9, 66]] = np.abs(M[2, [5, 9, 66]])
    M[:, 150] = M[:, 5]
    M[:, 70] = M[:, 66]
    true, x, y, th = make_poses(n, 6)
    x[:8], y[:8], th[:8] = true[0], true[1], true[2]   # (particles 0 .. 7 sit on the true pose: they match what it sees)
    zx, zy = make_detections(M, true, 20, 8)
    c, s = np.cos(true[2]), np.sin(true[2])
    for k, l in enumerate((5, 66, 9)):
        ddx, ddy = M[0, l] - true[0], M[1, l] - true[1]
        zx[k], zy[k] = c * ddx - s * ddy, s * ddx + c * ddy
    zx[7], zy[7] = zx[2], zy[2]
    zx[19], zy[19] = 1000.0, 1000.0
    covs = covariances(20, 9)
    for q in covs:
        q[7] = q[2]
    x[11] = np.nan
    _, m = AD.cost_matrix(M[None], x[20:21], y[20:21], th[20:21], None, zx, zy, covs)
    return M, x, y, th, zx, zy, covs, F(m[0, 66, 1])


def test_ties_gates_and_a_nan_pose(eng):
    M, x, y, th, zx, zy, covs, gate_on = tie_case()
    want, st, ll = check(eng, M, x, y, th, zx, zy, covs, label="ties")
    assert np.all(want[:, 150] == S.NONE) and np.all(want[:, 70] == S.NONE)   # the copies never win ...
    assert (want[:, 5] == 0).any() and (want[:, 66] == 1).any()        # ... their originals do: the lowest l
    assert np.all(want[:, 9] != 7) and (want[:, 9] == 2).any()         # the copy of detection 2 never wins landmark 9: the lowest k
    assert not (want == 19).any()                                      # outside every gate
    assert st[11, 0] == 0 and bits(ll[11:12])[0] == 0                  # the NaN pose: nothing matched, ll = +0
    assert np.isfinite(gate_on) and gate_on > 0
    want, _, _ = check(eng, M, x, y, th, zx, zy, covs, gate=gate_on, label="on the gate")
    assert want[20, 66] == 1                                           # m == gate is a candidate
    want, _, _ = check(eng, M, x, y, th, zx, zy, covs, gate=np.nextafter(gate_on, F(0)), label="just inside")
    assert want[20, 66] == S.NONE


def test_same_pose_same_bits(eng):
    """Two particles with one pose, at different wavefront positions of different workgroups."""
    n, L = 130, 129
    M = make_map(L, 21)
    true, x, y, th = make_poses(n, 22)
    for j in (1, 6, 67, 129):
        x[j], y[j], th[j] = x[0], y[0], th[0]
    zx, zy = make_detections(M, true, 17, 23)
    want, st, ll = check(eng, M, x, y, th, zx, zy, covariances(17, 24), label="same pose")
    for j in (1, 6, 67, 129):
        assert np.array_equal(want[j], want[0]) and np.array_equal(st[j], st[0]) and bits(ll[j:j + 1])[0] == bits(ll[:1])[0]


def test_largest_map(eng):
    """L = SLAM_MAX_OBS, 3 particles, K = 64: 64 batches, the path that reads the map from memory."""
    L = 8192
    M = make_map(L, 31)
    true, x, y, th = make_poses(3, 32)
    zx, zy = make_detections(M, true, 64, 33)
    _, st, _ = check(eng, M, x, y, th, zx, zy, covariances(64, 34), label="L=8192")
    assert st[:, 0].sum() > 0


def test_argument_checks_not_ready_and_the_counter(eng):
    L, Lp, n = 64, 64, 8
    M = make_map(L, 51)
    true, x, y, th = make_poses(n, 52)
    zx, zy = make_detections(M, true, 4, 53)
    covs = covariances(4, 54)
    pkg = load_package()
    before, iso_before = eng.localise_detcov_count(), eng.localise_counts()
    d_map = raw_map(M, Lp)
    run(eng, d_map, Lp, L, x, y, th, zx, zy, covs)
    assert eng.localise_detcov_count() == before + 1 and eng.localise_counts() == iso_before   # (in no other counter)
    d_st = torch.zeros((n, 3), dtype=torch.int32, device=DEV)
    d_tab = torch.zeros((n, L), dtype=torch.uint8, device=DEV)
    args = dict(plane_stride=Lp, nlandmarks=L, n=n, gate=GATE, assoc_stride=L)
    for bad in (dict(nlandmarks=0), dict(nlandmarks=8193), dict(plane_stride=L - 1), dict(gate=0.0), dict(gate=float("inf")),
                dict(gate=float("nan")), dict(n=-1), dict(assoc_stride=L - 1)):
        a = {**args, **bad}
        with pytest.raises(pkg.SlamError):
            eng.localise_detcov_dev(d_map, a["plane_stride"], a["nlandmarks"], dev(x), dev(y), dev(th), a["n"], a["gate"], d_tab,
                                    a["assoc_stride"], d_st, None)
    with pytest.raises(pkg.SlamError):
        eng.localise_detcov_dev(None, Lp, L, dev(x), dev(y), dev(th), n, GATE, d_tab, L, d_st, None)
    eng.detections_upload(zx, zy)   # detections without covariances
    with pytest.raises(pkg.SlamError) as err:
        eng.localise_detcov_dev(d_map, Lp, L, dev(x), dev(y), dev(th), n, GATE, d_tab, L, d_st, None)
    assert err.value.status == -4   # SLAM_ERR_NOT_READY
    assert eng.localise_detcov_count() == before + 1
