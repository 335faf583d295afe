"""slam_pose_reseed_dev (reseeding the cloud from what the lidar sees, csrc/reseed_kernels.hip) against the specification
tests/_reseed_spec.py: poses bit for bit, flags and counts exactly — at the smallest shapes at which the kernel can go wrong (one
slot, a wavefront less one, exactly one, one more, more than a workgroup, many workgroups with a ragged tail), both plane strides,
with and without empty slots, one detection and sixty-four, in place without a gather and out of place through one with duplicates
and a reversed order, every threshold, a particle id past 2^32, poses and landmarks out to 10^3 — and its refusals."""
import itertools

import numpy as np
import pytest
import torch

import _reseed_spec as R
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SEED = 0x0FED_CBA9_8765_4321
INVALID_ARG, NOT_READY = -2, -4


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


def make_map(L, empty, seed=21):
    """M [5][L] out to 10^3 m; empty: every third slot holds no landmark (L = 1: its only one)."""
    rng = np.random.default_rng(seed + L)
    M = np.zeros((5, L), F)
    M[0], M[1] = rng.uniform(-1000, 1000, (2, L)).astype(F)
    M[2], M[3], M[4] = 0.05, 0.01, 0.08
    if empty:
        M[2, ::3] = -1.0
    return M


def padded(M, Lp):
    raw = np.full((5, Lp), np.nan, F)   # the padding behind nlandmarks is never read: NaN would show
    raw[:, :M.shape[1]] = M
    return raw


def make_poses(n, seed=5):
    rng = np.random.default_rng(seed + n)
    return tuple(rng.uniform(-1000, 1000, n).astype(F) for _ in range(3))


def make_detections(K, seed=8):
    rng = np.random.default_rng(seed + K)
    return rng.uniform(-30, 30, K).astype(F), rng.uniform(-30, 30, K).astype(F)


def make_anc(n):
    """duplicates in the first half (every ancestor twice), a reversed order in the second"""
    a = np.arange(n, dtype=np.int32)[::-1].copy()
    a[: n // 2] = np.arange(n // 2, dtype=np.int32) // 2
    return a


def run(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction, flag=True):
    """-> (x', y', th', flag, counts): in place when anc is None, else into buffers of their own."""
    n, L = len(x), M.shape[1]
    Lp = (L + 31) // 32 * 32
    d_in = [dev(a) for a in (x, y, th)]
    d_out = d_in if anc is None else [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_flag = torch.full((n,), 9, dtype=torch.uint8, device=DEV) if flag else None
    eng.detections_upload(zx, zy)
    counts = eng.pose_reseed_dev(dev(padded(M, Lp)), Lp, L, *d_in, None if anc is None else dev(anc), *d_out, n, first_id, SEED, frame,
                                 fraction, d_flag)
    if anc is not None:   # the inputs are read only
        assert all(np.array_equal(bits(host(d)), bits(a)) for d, a in zip(d_in, (x, y, th)))
    return [host(d) for d in d_out] + [host(d_flag) if flag else None, counts]


def check(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction, label):
    want = R.reseed(M, x, y, th, anc, zx, zy, first_id, SEED, frame, fraction)
    got = run(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction)
    for k, name in enumerate(("x", "y", "theta")):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{label}: {name} differs at {np.flatnonzero(bits(got[k]) != bits(want[k]))[:5].tolist()}"
    assert np.array_equal(got[3], want[3]), f"{label}: flags"
    assert got[4] == tuple(want[4]), f"{label}: counts {got[4]} != {tuple(want[4])}"
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4099])
def test_stage_equals_the_spec(eng, n):
    x, y, th = make_poses(n)
    anc = make_anc(n)
    replaced = empty_seen = kept = 0
    cases = itertools.product((1, 33), (False, True), (1, 64), (False, True), (1.0, 0.5, 2.0**-10), (0, 2**32 + 7))
    for frame, (L, empty, K, gather, fraction, first_id) in enumerate(cases):
        M = make_map(L, empty)
        zx, zy = make_detections(K)
        want = check(eng, M, x, y, th, anc if gather else None, zx, zy, first_id, frame, fraction,
                     f"n {n} L {L} empty {empty} K {K} gather {gather} fraction {fraction} first_id {first_id}")
        replaced += int(want[4][0])
        empty_seen += int(want[4][1])
        kept += n - int(want[4].sum())
    assert replaced > 0 and empty_seen > 0 and kept > 0   # every branch of a slot was taken


def test_many_workgroups_count_exactly(eng):
    """65 536 slots are 256 workgroups: the counts are the sums of every workgroup's, and the accumulators are left clean for the
    call behind it (the same launch again gives the same counts)."""
    n = 65536
    x, y, th = make_poses(n)
    M = make_map(33, True)
    zx, zy = make_detections(64)
    c0 = eng.pose_reseed_count()
    for frame in (3, 3, 4):
        want = check(eng, M, x, y, th, make_anc(n), zx, zy, 2**32 + 7, frame, 0.5, f"frame {frame}")
        assert want[4][0] > n // 4 and want[4][1] > n // 16
    assert eng.pose_reseed_count() - c0 == 3
    got = run(eng, M, x, y, th, None, zx, zy, 0, 5, 0.5, flag=False)   # no flag pointer
    want = R.reseed(M, x, y, th, None, zx, zy, 0, SEED, 5, 0.5)
    assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in range(3)) and got[4] == tuple(want[4])


def test_refusals(eng):
    pkg = load_package()
    n, L, Lp = 64, 5, 32
    x, y, th = make_poses(n)
    d_map = dev(padded(make_map(L, False), Lp))
    d_in = [dev(a) for a in (x, y, th)]
    d_out = [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_anc = dev(make_anc(n))
    d_big = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    eng.detections_upload(*make_detections(4))
    c0 = eng.pose_reseed_count()

    def call(map_=d_map, ps=Lp, nl=L, ins=d_in, anc=None, outs=d_out, n_=n, fraction=0.5):
        return eng.pose_reseed_dev(map_, ps, nl, *ins, anc, *outs, n_, 0, SEED, 0, fraction)

    bad = [dict(n_=0), dict(n_=-3), dict(nl=0), dict(nl=-1), dict(ps=L - 1), dict(fraction=0.0), dict(fraction=-0.25), dict(fraction=1.5),
           dict(fraction=float("nan")), dict(fraction=float("inf")), dict(map_=None), dict(ins=[None, d_in[1], d_in[2]]),
           dict(outs=[d_out[0], None, d_out[2]]),
           dict(anc=d_anc, outs=d_in),                                        # in place through a gather
           dict(outs=[d_in[1], d_out[1], d_out[2]]),                          # x_out is y_in
           dict(ins=[d_big[:n], d_big[n:2 * n], d_big[2 * n:3 * n]], outs=[d_big[1:n + 1], d_out[1], d_out[2]]),   # shifted by one float
           dict(anc=d_anc, ins=[d_big[:n], d_big[n:2 * n], d_big[2 * n:3 * n]], outs=[d_big[n - 1:2 * n - 1], d_out[1], d_out[2]])]
    for kw in bad:
        with pytest.raises(pkg.SlamError) as err:
            call(**kw)
        assert err.value.status == INVALID_ARG, kw
    assert eng.pose_reseed_count() == c0 and all(np.all(host(d) == 7.0) for d in d_out)
    assert sum(call()) > 0 and eng.pose_reseed_count() == c0 + 1                  # the good call, out of place without a gather
    assert sum(call(anc=d_anc)) > 0 and sum(call(outs=d_in)) > 0                 # ... through one; in place without

    fresh = pkg.Engine(0)   # no detections were ever handed over
    with pytest.raises(pkg.SlamError) as err:
        fresh.pose_reseed_dev(d_map, Lp, L, *d_in, None, *d_out, n, 0, SEED, 0, 0.5)
    assert err.value.status == NOT_READY
    with pytest.raises(pkg.SlamError) as err:   # ... and an invalid argument is still one
        fresh.pose_reseed_dev(d_map, Lp, L, *d_in, None, *d_out, 0, 0, SEED, 0, 0.5)
    assert err.value.status == INVALID_ARG
    torch.cuda.synchronize()
    fresh.close()


def test_no_detections_write_nothing(eng):
    n, L, Lp = 257, 5, 32
    x, y, th = make_poses(n)
    d_out = [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_flag = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    eng.detections_upload(np.zeros(0, F), np.zeros(0, F))
    c0 = eng.pose_reseed_count()
    counts = eng.pose_reseed_dev(dev(padded(make_map(L, False), Lp)), Lp, L, dev(x), dev(y), dev(th), None, *d_out, n, 0, SEED, 0, 1.0, d_flag)
    assert counts == (0, 0) and eng.pose_reseed_count() == c0
    assert all(np.all(host(d) == 7.0) for d in d_out) and np.all(host(d_flag) == 9)
