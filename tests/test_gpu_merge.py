"""slam_landmark_merge_dev (csrc/merge_kernels.hip) against its specification tests/_merge_spec.py: map rows, evidence bytes and
stats bit for bit whatever the shape, the strides (the table's dword and byte path), the number of detections and of anchors, with
evidence and without; the branch cases of tests/_merge_cases.py per particle; the argument checks launch nothing."""
import numpy as np
import pytest
import torch

import _merge_cases as MC
import _merge_spec as M
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GATE, CMAX = 9.0, 200
G = 16   # guard bytes around the byte arrays


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def run_case(eng, n, L, plane_stride, assoc_stride, ev_stride, K, anchors, seed, with_ev=True, offset=0, label=""):
    """One launch against the spec; the byte arrays sit `offset` bytes off a dword inside guard bytes that must not change.
    -> the spec's stats summed over the particles (merged, refused, seen after)."""
    mp, tab, c, kind = MC.make_case(n, L, plane_stride, K, anchors, seed)

    def guarded(arr, stride, s):
        flat = np.random.default_rng(seed + s).integers(0, 256, 2 * G + offset + n * stride).astype(np.uint8)
        flat[G + offset:G + offset + n * stride].reshape(n, stride)[:, :L] = arr
        return flat

    body = lambda flat, stride: flat[G + offset:G + offset + n * stride].reshape(n, stride)
    h_tab, h_ev = guarded(tab, assoc_stride, 2), guarded(c, ev_stride, 3)
    want_mp, want_ev, want_st = M.merge(mp, body(h_tab, assoc_stride), K, GATE, body(h_ev, ev_stride) if with_ev else None,
                                        CMAX if with_ev else None, L=L)
    want_flat = h_ev.copy()
    if with_ev:
        body(want_flat, ev_stride)[:] = want_ev
    d_mp, d_tab, d_ev = dev(mp), dev(h_tab), dev(h_ev)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    eng.detections_upload(np.zeros(K, F), np.zeros(K, F))
    at = G + offset
    eng.landmark_merge_dev(d_mp, 5 * plane_stride, plane_stride, L, n, d_tab[at:], assoc_stride, d_ev[at:] if with_ev else None, ev_stride,
                           CMAX, GATE, d_st)
    got_st, got_mp, got_ev = host(d_st), host(d_mp), host(d_ev)
    assert np.array_equal(got_st, want_st), f"{label}: stats differ at {np.argwhere(got_st != want_st)[:5].tolist()}"
    assert np.array_equal(bits(got_mp), bits(want_mp)), f"{label}: map rows differ at {np.argwhere(bits(got_mp) != bits(want_mp))[:5].tolist()}"
    assert np.array_equal(got_ev, want_flat), f"{label}: evidence differs at {np.argwhere(got_ev != want_flat)[:5].ravel().tolist()}"
    assert np.array_equal(host(d_tab), h_tab), f"{label}: the table changed"
    return want_st.sum(axis=0)


def strides(L):
    """(plane_stride, assoc_stride, ev_stride, offset): L rounded up to 32 everywhere (the dword path); a plane stride and byte
    strides that are no multiple of 4 (the byte path); dword strides on a base that is off a dword (the byte path)."""
    Lp, L4 = (L + 31) // 32 * 32, (L + 3) // 4 * 4
    odd = L + 1 if (L + 1) % 2 else L + 2
    return ((Lp, Lp, Lp, 0), (Lp + 3, odd, odd + 2, 0), (Lp, L4, L4 + 4, 1))


@pytest.mark.parametrize("L", [1, 2, 63, 64, 65, 128, 129, 200])
def test_stage_equals_the_spec(eng, L):
    c0 = eng.merge_count()
    launches, total = 0, np.zeros(3, np.int64)
    for j, (ps, ts, es, offset) in enumerate(strides(L)):
        for k, (K, anchors) in enumerate(((0, 0), (1, 1), (4, 4), (4, 0), (64, 1), (64, 64))):
            n = (1, 5, 5)[(j + k) % 3]
            total += run_case(eng, n, L, ps, ts, es, K, anchors, seed=1000 * L + 10 * j + k, with_ev=(j + k) % 2 == 0, offset=offset,
                              label=f"L={L} strides {j} K={K} anchors={anchors}")
            launches += 1
    eng.sync()
    assert eng.merge_count() == c0 + launches
    if L >= 2:
        assert total[0] > 0, total
    if L >= 128:
        assert total[1] > 0, total


def test_several_workgroups(eng):
    """n = 257: more than 64 workgroups and a last one that is not full; L = 37 is no multiple of anything."""
    for j, (ps, ts, es, offset, K, anchors, with_ev) in enumerate(((64, 64, 64, 0, 4, 4, True), (39, 37, 41, 0, 64, 20, True),
                                                                    (64, 40, 40, 1, 4, 4, False))):
        total = run_case(eng, 257, 37, ps, ts, es, K, anchors, seed=7 + j, with_ev=with_ev, offset=offset, label=f"n=257 {j}")
        assert total[0] > 0 and (j != 1 or total[1] > 0), total


def test_a_table_that_names_a_detection_twice(eng):
    """More than 64 named slots: the first 64 are the anchors, the others take no part — and nothing is written out of bounds."""
    n, L, Lp = 5, 200, 224
    mp, tab, c, _ = MC.make_case(n, L, Lp, 64, 64, seed=5)
    tab[:, ::2] = np.where(tab[:, ::2] == 255, 3, tab[:, ::2])         # every other free slot is named too: about 130 named per particle
    assert ((tab < 64) & ~(mp[:, 2, :L] < 0)).sum(axis=1).min() > 64
    want_mp, want_ev, want_st = M.merge(mp, tab, 64, GATE, c, CMAX, L=L)
    d_mp, d_tab, d_ev = dev(mp), dev(tab), dev(c)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    eng.detections_upload(np.zeros(64, F), np.zeros(64, F))
    eng.landmark_merge_dev(d_mp, 5 * Lp, Lp, L, n, d_tab, L, d_ev, L, CMAX, GATE, d_st)
    assert np.array_equal(host(d_st), want_st) and np.array_equal(bits(host(d_mp)), bits(want_mp)) and np.array_equal(host(d_ev), want_ev)
    assert want_st[:, 0].sum() > 0


def test_argument_checks_launch_nothing(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    mp, tab, c, _ = MC.make_case(n, L, Lp, 4, 4, seed=3)
    d_mp = dev(mp)
    d_tab = torch.full((n, Lp), 255, dtype=torch.uint8, device=DEV)
    d_tab[:, :L] = dev(tab)
    d_ev = torch.full((n, Lp), 5, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    ok = dict(mp=d_mp, ps=Lp, L=L, n=n, tab=d_tab, ts=Lp, ev=d_ev, es=Lp, cmax=8, gate=GATE, st=d_st)

    def call(e, **change):
        a = dict(ok, **change)
        e.landmark_merge_dev(a["mp"], a.get("rs", 5 * a["ps"]), a["ps"], a["L"], a["n"], a["tab"], a["ts"], a["ev"], a["es"], a["cmax"], a["gate"],
                             a["st"])

    fresh = pkg.Engine(0)
    with pytest.raises(pkg.SlamError) as err:                       # no detections handed over
        call(fresh)
    assert err.value.status == -4 and fresh.merge_count() == 0
    fresh.close()
    eng.detections_upload(np.zeros(4, F), np.zeros(4, F))
    c0 = eng.merge_count()
    nan, inf = float("nan"), float("inf")
    for change in (dict(gate=0.0), dict(gate=-1.0), dict(gate=nan), dict(gate=inf), dict(gate=-inf), dict(ps=L - 1), dict(ts=L - 1), dict(es=L - 1),
                   dict(rs=5 * Lp - 1), dict(L=8193, ps=8200, ts=8200, es=8200), dict(L=-1), dict(n=-1), dict(cmax=0), dict(cmax=256), dict(cmax=-1),
                   dict(mp=None), dict(tab=None)):
        with pytest.raises(pkg.SlamError) as err:
            call(eng, **change)
        assert err.value.status == -2, change
    eng.sync()
    # nothing was launched
    assert eng.merge_count() == c0 and np.all(host(d_ev) == 5) and np.all(host(d_st) == -1) and np.array_equal(bits(host(d_mp)), bits(mp))
    call(eng, st=None)                                              # no stats wanted
    call(eng, ev=None, es=0, cmax=0)                                # without evidence its stride and cmax are not read
    call(eng, n=0)                                                  # nothing to do: no launch
    eng.sync()
    assert eng.merge_count() == c0 + 2
    eng.detections_upload(np.zeros(0, F), np.zeros(0, F))           # K = 0 is legal: no anchors, nothing happens, seen is counted
    d_mp2 = dev(mp)
    call(eng, mp=d_mp2)
    assert np.array_equal(bits(host(d_mp2)), bits(mp)) and np.array_equal(host(d_st)[:, :2], np.zeros((n, 2), np.int32))
    assert np.array_equal(host(d_st)[:, 2], (~(mp[:, 2, :L] < 0)).sum(axis=1))
