"""slam_known_map_prepare_dev / slam_localise_dev (localisation in a known map, csrc/localise_kernels.hip) against the specification
tests/_localise_spec.py: the table's bytes, the stats and the log-likelihood's bits are equal exactly — whatever the shape, with
unseen slots scattered through the map, ties between landmarks and between detections, a detection outside every gate and one
exactly on it, a NaN pose, with and without a table pointer, on the staged and on the unstaged path."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
import _localise_spec as S
import oracle
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
Q, GATE = 0.02, 9.21
F = np.float32


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for torch's fills and copies and the engine's launches
    yield e
    torch.cuda.synchronize()
    e.close()


def make_map(L, seed, unseen=0.2):
    """M [5][L]: poles scattered over a 40 m square, covariances of a few centimetres with a correlation, and a share of slots
    that hold no landmark (P_xx = -1) scattered through it."""
    rng = np.random.default_rng(seed)
    M = np.zeros((5, L), np.float32)
    M[0], M[1] = rng.uniform(-20, 20, L), rng.uniform(-20, 20, L)
    sx, sy, r = rng.uniform(0.02, 0.3, L), rng.uniform(0.02, 0.3, L), rng.uniform(-0.8, 0.8, L)
    M[2], M[3], M[4] = sx * sx, r * sx * sy, sy * sy
    if L > 1:
        M[2, rng.random(L) < unseen] = -1.0
    return M


def make_poses(n, seed):
    """A true pose and a cloud around it, tight enough that many particles match and loose enough that many do not."""
    rng = np.random.default_rng(seed)
    true = np.array([1.5, -2.0, 0.7], np.float32)
    x = (true[0] + 0.15 * rng.standard_normal(n)).astype(F)
    y = (true[1] + 0.15 * rng.standard_normal(n)).astype(F)
    th = (true[2] + 0.02 * rng.standard_normal(n)).astype(F)
    return true, x, y, th


def make_detections(M, true, K, seed):
    """K sensor-frame points: the seen landmarks nearest the true pose as it would see them (shuffled, a little noise), and once
    those run out points that belong to nothing."""
    rng = np.random.default_rng(seed)
    seen = np.flatnonzero(~(M[2] < 0))
    d = np.hypot(M[0, seen] - true[0], M[1, seen] - true[1])
    pick = rng.permutation(seen[np.argsort(d)][:K])
    c, s = np.cos(true[2]), np.sin(true[2])
    dx, dy = M[0, pick] - true[0], M[1, pick] - true[1]
    # z = H (m - t), H = [[c, -s], [s, c]]: the observation model of the landmark update (w = t + H^T z gives m back)
    zx = np.concatenate([c * dx - s * dy + 0.02 * rng.standard_normal(len(pick)), rng.uniform(-30, 30, K - len(pick))])
    zy = np.concatenate([s * dx + c * dy + 0.02 * rng.standard_normal(len(pick)), rng.uniform(-30, 30, K - len(pick))])
    return zx.astype(F), zy.astype(F)


def prepare(eng, M, Lp, q=Q):
    L = M.shape[1]
    raw = np.zeros((5, Lp), np.float32)
    raw[2] = -1.0
    raw[:, :L] = M
    d_prep = torch.full((6, Lp), 3.0, dtype=torch.float32, device=DEV)
    eng.known_map_prepare_dev(dev(raw), Lp, L, q, d_prep)
    return d_prep


def run(eng, d_prep, Lp, L, x, y, th, zx, zy, gate=GATE, table=True, stride=None):
    n = len(x)
    stride = L if stride is None else stride
    d_assoc = torch.full((n, stride), 7, dtype=torch.uint8, device=DEV) if table else None
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    d_ll = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
    eng.detections_upload(zx, zy)
    eng.localise_dev(d_prep, Lp, L, dev(x), dev(y), dev(th), n, gate, d_assoc, stride, d_st, d_ll)
    return (host(d_assoc) if table else None), host(d_st), host(d_ll)


def check(eng, M, x, y, th, zx, zy, gate=GATE, stride=None, label=""):
    """Prepare + one launch against the spec: table (the whole stride), stats, ll bits; then the same without a table pointer."""
    L = M.shape[1]
    Lp = (L + 31) // 32 * 32
    stride = L if stride is None else stride
    want, want_st, want_ll = S.localise(M, x, y, th, zx, zy, Q, gate, 0.0)
    want = np.concatenate([want, np.full((len(x), stride - L), A.NONE, np.uint8)], axis=1)
    d_prep = prepare(eng, M, Lp)
    got, got_st, got_ll = run(eng, d_prep, Lp, L, x, y, th, zx, zy, gate, True, stride)
    assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: ll differs at {np.flatnonzero(bits(got_ll) != bits(want_ll))[:5].tolist()}"
    _, st2, ll2 = run(eng, d_prep, Lp, L, x, y, th, zx, zy, gate, False)
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
    _, st, ll = check(eng, M, x, y, th, zx, zy, stride=(L + 35) // 32 * 32 if K % 2 == 0 else L + 3, label=f"L={L} K={K}")
    assert np.all(st[:, 1] == 0) and np.all(st.sum(axis=1) == K)
    if K == 0:
        assert np.all(bits(ll) == 0)   # +0
    if K >= 17 and L >= 64:
        assert 0 < st[:, 0].sum() < n * K   # (the case exercises both outcomes)


def tie_case():
    """-> (M, x, y, th, zx, zy, gate_on): landmarks 150 and 70 are bit-identical copies of 5 and 66, detection 7 of detection 2;
    detection 19 lies outside every gate; particle 11 has x = NaN; gate_on is the cost of (particle 20, landmark 66, detection 1)
    by the spec's own operations: with it as the gate that pair lies exactly ON the gate."""
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
    x[11] = np.nan
    sc, cc = oracle.det_sincos(th[20:21])
    wx, wy = A.observed_point(zx[1], zy[1], sc, cc, x[20:21], y[20:21])
    with np.errstate(all="ignore"):
        m = A.cost(A.shared(M[None], Q), wx[:, None], wy[:, None])[0]
    return M, x, y, th, zx, zy, F(m[66])


def test_ties_gates_and_a_nan_pose(eng):
    M, x, y, th, zx, zy, gate_on = tie_case()
    want, st, ll = check(eng, M, x, y, th, zx, zy, label="ties")
    assert np.all(want[:, 150] == A.NONE) and np.all(want[:, 70] == A.NONE)   # the copies never win ...
    assert (want[:, 5] == 0).any() and (want[:, 66] == 1).any()        # ... their originals do: the lowest l
    assert np.all(want[:, 9] != 7) and (want[:, 9] == 2).any()         # the copy of detection 2 never wins landmark 9: the lowest k
    assert not (want == 19).any()                                      # outside every gate
    assert st[11, 0] == 0 and bits(ll[11:12])[0] == 0                  # the NaN pose: nothing matched, ll = +0
    assert np.isfinite(gate_on) and gate_on > 0
    want, _, _ = check(eng, M, x, y, th, zx, zy, gate=gate_on, label="on the gate")
    assert want[20, 66] == 1                                           # m == gate is a candidate
    want, _, _ = check(eng, M, x, y, th, zx, zy, gate=np.nextafter(gate_on, F(0)), label="just inside")
    assert want[20, 66] == A.NONE


def test_same_pose_same_bits(eng):
    """Two particles with one pose, at different wavefront positions of different workgroups."""
    n, L = 130, 129
    M = make_map(L, 21)
    true, x, y, th = make_poses(n, 22)
    for j in (1, 6, 67, 129):
        x[j], y[j], th[j] = x[0], y[0], th[0]
    zx, zy = make_detections(M, true, 17, 23)
    want, st, ll = check(eng, M, x, y, th, zx, zy, label="same pose")
    for j in (1, 6, 67, 129):
        assert np.array_equal(want[j], want[0]) and np.array_equal(st[j], st[0]) and bits(ll[j:j + 1])[0] == bits(ll[:1])[0]


def test_largest_map(eng):
    """L = SLAM_MAX_OBS, 3 particles, K = 64: 64 batches, the path that reads the prepared map from memory."""
    L = 8192
    M = make_map(L, 31)
    true, x, y, th = make_poses(3, 32)
    zx, zy = make_detections(M, true, 64, 33)
    _, st, _ = check(eng, M, x, y, th, zx, zy, label="L=8192")
    assert st[:, 0].sum() > 0


def test_prepare_equals_the_spec(eng):
    """Plane by plane: _assoc_spec.shared for S^-1, the oracle's logarithm for hl; slots without a landmark and the padding carry a
    NaN mean."""
    L, Lp = 200, 224
    M = make_map(L, 41)
    got = host(prepare(eng, M, Lp))
    seen, mx, my, i00, i01, i11 = (a[0] for a in A.shared(M[None], Q))
    a, c = M[2] + F(Q), M[4] + F(Q)
    det = a * c - M[3] * M[3]
    hl = F(0.5) * oracle.det_log(det[seen])
    assert 0 < seen.sum() < L
    for p, want in enumerate((mx, my, i00, i01, i11)):
        assert np.array_equal(bits(got[p, :L][seen]), bits(want[seen])), f"plane {p}"
    assert np.array_equal(bits(got[5, :L][seen]), bits(hl)), "hl"
    assert np.all(np.isnan(got[0, :L][~seen])) and np.all(np.isnan(got[0, L:]))


def test_argument_checks_and_counts(eng):
    L, Lp, n = 64, 64, 8
    M = make_map(L, 51)
    true, x, y, th = make_poses(n, 52)
    zx, zy = make_detections(M, true, 4, 53)
    pkg = load_package()
    before = eng.localise_counts()
    d_prep = prepare(eng, M, Lp)
    run(eng, d_prep, Lp, L, x, y, th, zx, zy)
    assert eng.localise_counts() == (before[0] + 1, before[1] + 1)
    d_st = torch.zeros((n, 3), dtype=torch.int32, device=DEV)
    args = dict(plane_stride=Lp, nlandmarks=L, n=n, gate=GATE, assoc_stride=L)
    for bad in (dict(nlandmarks=0), dict(nlandmarks=8193), dict(plane_stride=L - 1), dict(gate=0.0), dict(gate=float("inf")),
                dict(gate=float("nan")), dict(n=-1), dict(assoc_stride=L - 1)):
        a = {**args, **bad}
        with pytest.raises(pkg.SlamError):
            eng.localise_dev(d_prep, a["plane_stride"], a["nlandmarks"], dev(x), dev(y), dev(th), a["n"], a["gate"],
                             torch.zeros((n, L), dtype=torch.uint8, device=DEV), a["assoc_stride"], d_st, None)
    with pytest.raises(pkg.SlamError):
        eng.known_map_prepare_dev(dev(M), L, L, 0.0, d_prep)
    assert eng.localise_counts() == (before[0] + 1, before[1] + 1)
