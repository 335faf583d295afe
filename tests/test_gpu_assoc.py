"""slam_associate_dev (data association, csrc/assoc_kernels.hip) against its specification tests/_assoc_spec.py: the table's bytes
and the stats are equal exactly, whatever the shape, the gather index, the padding, ties, NaN priors and the number of unseen
slots; the source rows are not written; the argument checks and the counters."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
from _detections import detections   # noqa: F401 - other tests import it from here
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_aniso import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 3, 65, 1000)
LS = (1, 31, 64, 65, 128, 129, 500)
KS = (0, 1, 7, 64)
Q, GATE, NEW_GATE = 0.02, 9.21, 50.0


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


def check(eng, poses, rows, L, dx, dy, anc=None, stride=None, gate=GATE, new_gate=NEW_GATE, create=1, label=""):
    """One launch against the spec: table bytes (the whole stride) and stats; -> (table, stats)."""
    x, y, th = poses
    n, Lp = len(x), rows.shape[2]
    stride = L if stride is None else stride
    want, want_st = A.associate(rows, x, y, th, anc, dx, dy, Q, gate, new_gate, create, L=L, assoc_stride=stride)
    d_rows = dev(rows)
    d_assoc = torch.full((n, stride), 7, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    eng.detections_upload(dx, dy)
    eng.associate_dev(d_rows, 5 * Lp, Lp, L, dev(x), dev(y), dev(th), dev(anc) if anc is not None else None, n, Q, gate, new_gate,
                      create, d_assoc, stride, d_st)
    got, got_st = host(d_assoc), host(d_st)
    assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(bits(host(d_rows)), bits(rows)), f"{label}: the source rows changed"
    return want, want_st


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_table_equals_the_spec(eng, n, L):
    """Every K, with and without a gather index of repeated, out-of-order ancestors; the stride leaves padding columns (every
    other K: a stride that is no multiple of 4, the byte path of the write-out)."""
    Lp = (L + 31) // 32 * 32
    poses, rows, zx, zy = make_case(n, L, Lp, 1000 * n + L)
    anc = np.random.default_rng(n + L).integers(0, n, n).astype(np.int32)
    matched = created = 0
    for j, K in enumerate(KS):
        dx, dy = detections(zx, zy, K, K)
        for a in (None, anc):
            _, st = check(eng, poses, rows, L, dx, dy, anc=a, stride=Lp if j % 2 == 0 else L + 3, label=f"n={n} L={L} K={K} anc={a is not None}")
            matched += int(st[:, 0].sum())
            created += int(st[:, 1].sum())
    if n >= 65 and L >= 31:
        assert matched > 0 and created > 0   # (the cases exercise both outcomes)


def test_longest_row(eng):
    """L = SLAM_MAX_OBS: the largest LDS carve, 64 batches."""
    L = 8192
    poses, rows, zx, zy = make_case(3, L, L, 4)
    dx, dy = detections(zx, zy, 64, 1)
    _, st = check(eng, poses, rows, L, dx, dy, anc=np.array([2, 0, 2], np.int32), label="L=8192")
    assert st[:, 0].sum() > 0


def test_ties_go_to_the_lowest_index(eng):
    n, L, Lp = 65, 129, 160
    poses, rows, zx, zy = make_case(n, L, Lp, 11)
    rows[:, 2, :L] = np.abs(rows[:, 2, :L])                       # everything seen
    # two bit-identical landmarks, in different batches of 64 lanes: the detection must take the lower one
    rows[:, :, 100] = rows[:, :, 5]
    rows[:, :, 70] = rows[:, :, 66]
    dx, dy = detections(zx, zy, 20, 3)
    dx[:3], dy[:3] = zx[[5, 66, 9]], zy[[5, 66, 9]]
    # two bit-identical detections: the landmark must take the lower one
    dx[7], dy[7] = dx[2], dy[2]
    want, _ = check(eng, poses, rows, L, dx, dy, label="ties")
    took5, took66, took9 = (want[:, l] != A.NONE for l in (5, 66, 9))
    assert took5.any() and took66.any() and took9.any()
    assert np.all(want[:, 100] != 0) and np.all(want[:, 70] != 1)  # the copies never win their detection ...
    assert not np.any(want == 7)                                   # ... and the copy of a detection is never chosen


def test_edge_cases(eng):
    n, L, Lp = 65, 129, 160
    poses, rows, zx, zy = make_case(n, L, Lp, 12)
    dx, dy = detections(zx, zy, 33, 5)
    _, st = check(eng, poses, rows, L, dx, dy, gate=1e-12, new_gate=1e-12, label="tiny gate")
    assert np.all(st[:, 0] == 0) and st[:, 1].sum() > 0
    _, st = check(eng, poses, rows, L, dx, dy, create=0, label="create = 0")
    assert np.all(st[:, 1] == 0) and st[:, 0].sum() > 0
    nanp = rows.copy()
    nanp[:, 3, 0:L:4] = np.nan                                     # a NaN covariance: seen, never a candidate, never near
    nanp[::2, 2, 1:L:4] = np.nan
    check(eng, poses, nanp, L, dx, dy, label="NaN priors")
    unseen = rows.copy()
    unseen[:, 2, :L] = -1.0
    _, st = check(eng, poses, unseen, L, dx, dy, label="all unseen")
    assert np.all(st == [0, 33, 0])
    _, st = check(eng, poses, unseen, 20, dx, dy, stride=32, label="all unseen, slots run out")
    assert np.all(st == [0, 20, 13])
    seen = rows.copy()
    seen[:, 2, :L] = np.abs(seen[:, 2, :L])
    _, st = check(eng, poses, seen, L, dx, dy, label="none unseen")
    assert np.all(st[:, 1] == 0) and st[:, 2].sum() > 0
    _, st = check(eng, poses, rows, L, dx, dy, new_gate=float("inf"), label="new_gate = inf")


def test_argument_checks_and_counters(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 3)
    d_rows, d_assoc = dev(rows), torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    pose = (dev(x), dev(y), dev(th))
    fresh = pkg.Engine(0)
    with pytest.raises(pkg.SlamError) as err:                       # no detections handed over
        fresh.associate_dev(d_rows, 5 * Lp, Lp, L, *pose, None, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, None)
    assert err.value.status == -4
    with pytest.raises(pkg.SlamError) as err:
        fresh.ekf_update_assoc_dev(d_rows, torch.empty_like(d_rows), 5 * Lp, Lp, L, *pose, None, n, Q, d_assoc, Lp, None)
    assert err.value.status == -4
    fresh.close()
    for bad in ((np.array([np.nan], np.float32), np.zeros(1, np.float32)), (np.zeros(1, np.float32), np.array([np.inf], np.float32)),
                (np.zeros(65, np.float32), np.zeros(65, np.float32))):
        with pytest.raises(pkg.SlamError) as err:
            eng.detections_upload(*bad)
        assert err.value.status == -2
    eng.detections_upload(zx[:5], zy[:5])
    c0, f0, i0 = eng.assoc_counts(), eng.ekf_form_counts(), eng.ekf_inplace_form_counts()
    ok = dict(meas_var=Q, gate=GATE, new_gate=NEW_GATE, create=1, L=L, stride=Lp, anc=None)
    for change in (dict(gate=0.0), dict(gate=-1.0), dict(gate=float("nan")), dict(gate=float("inf")), dict(new_gate=GATE / 2),
                   dict(new_gate=float("nan")), dict(meas_var=0.0), dict(meas_var=-1.0), dict(L=8193, stride=8193), dict(stride=L - 1),
                   dict(create=2)):
        a = dict(ok, **change)
        with pytest.raises(pkg.SlamError) as err:
            eng.associate_dev(d_rows, 5 * max(Lp, a["L"]), max(Lp, a["L"]), a["L"], *pose, a["anc"], n, a["meas_var"], a["gate"], a["new_gate"],
                              a["create"], d_assoc, a["stride"], None)
        assert err.value.status == -2, change
    d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
    d_anc = dev(np.zeros(n, np.int32))
    for call in (lambda: eng.ekf_update_assoc_dev(d_rows, d_rows, 5 * Lp, Lp, L, *pose, d_anc, n, Q, d_assoc, Lp, None),   # gather in place
                 lambda: eng.ekf_update_assoc_dev(d_rows, d_out, 5 * Lp, Lp, L, *pose, None, n, Q, d_assoc, L - 1, None),
                 lambda: eng.ekf_update_assoc_dev(d_rows, d_out, 5 * Lp, Lp, L, *pose, None, n, 0.0, d_assoc, Lp, None),
                 lambda: eng.ekf_update_assoc_dev(d_rows, d_out, 5 * 8200, 8200, 8193, *pose, None, n, Q, d_assoc, 8200, None)):
        with pytest.raises(pkg.SlamError) as err:
            call()
        assert err.value.status == -2
    assert eng.assoc_counts() == c0 and np.all(host(d_assoc) == 7) and np.all(host(d_out) == 7.0)   # nothing was launched
    eng.associate_dev(d_rows, 5 * Lp, Lp, L, *pose, None, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, None)   # (no stats wanted)
    eng.ekf_update_assoc_dev(d_rows, d_out, 5 * Lp, Lp, L, *pose, None, n, Q, d_assoc, Lp, None)
    eng.sync()
    assert eng.assoc_counts() == (c0[0] + 1, c0[1] + 1)
    assert eng.ekf_form_counts() == f0 and eng.ekf_inplace_form_counts() == i0
