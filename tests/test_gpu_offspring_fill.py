"""offspring_fill_kernel (csrc/resample_kernels.hip): every particle computes the run of slots it owns from two neighbouring
CDF values and writes its own index into it; the wavefront fills the long runs together.  The ancestors of every slot against
the exact integers of tests/_resample_exact.py, element for element, at the sizes where a lane, a wavefront, a workgroup or a
2048-element tile ends (and one at the top of the range whose tile totals one turn of the workgroup reads, one above it):
equal weights (runs of length 1), one particle with all the weight at 0, n / 2 and n - 1 (one run of n: the wavefront's fill
and the last particle's rule), the same with a few units of weight on everyone else, two survivors on both sides of a wavefront,
a workgroup and a tile edge (equal and unequal shares), a geometric ramp (runs of every length on both sides of the
owner-stores / wavefront-stores threshold), and the structured catalogue, each at several frames (the comb offset moves).
With them the survivor marks (mark[i] == stamp iff i is somebody's ancestor; through slam_ancestors_survivors_dev, which the
session calls and the Python binding does not carry), a gated frame that keeps its population (ancestor j of slot j, everybody
marked), and one C session against the CPU specification loop with its rows read through the pending gather.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import _resample_exact as X
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED = 0x1234567887654321
FRAMES = (0, 5, 123457)
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4099, 6149]
GUARD = 128


class SurvivorOut(C.Structure):   # csrc/kernels.h
    _fields_ = [("mark", C.c_void_p), ("stamp", C.c_uint32)]


@pytest.fixture(scope="module")
def engines():
    """(plain, gated): the gate's flag and carried weights live in the engine"""
    pkg = load_package()
    both = [pkg.Engine(0), pkg.Engine(0)]
    for e in both:
        e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield both
    torch.cuda.synchronize()
    for e in both:
        e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def _carriers(n, spots, logws):
    lw = np.full(n, X.ZERO, np.float32)
    for i, v in zip(spots, logws):
        lw[i] = np.float32(v)
    return lw


def own_populations(n):
    """name -> (log-weights, outside maximum or None)"""
    out = {"all_equal": (np.full(n, X.CARRIER, np.float32), None)}
    for i in sorted({0, n // 2, n - 1}):
        out[f"only@{i}"] = (_carriers(n, [i], [0.0]), None)
        lw = np.full(n, X.TINY, np.float32)
        lw[i] = X.CARRIER
        out[f"dominant@{i}"] = (lw, None)
    for edge in (64, 256, 2048):   # two survivors whose owners sit on both sides of the edge; the run boundary falls mid-population
        if edge < n:
            out[f"pair@{edge}"] = (_carriers(n, [edge - 1, edge], [0.0, 0.0]), None)
            out[f"pair@{edge},unequal"] = (_carriers(n, [edge - 1, edge], [-1.25, 0.0]), None)
            if 2 * edge < n:   # ... and whose runs meet near slot `edge`: the second one is rest / edge times as heavy
                out[f"pair_meets@{edge}"] = (_carriers(n, [0, n - 1], [np.log(edge / (n - edge)), 0.0]), None)
    out["ramp"] = (np.maximum(np.float32(-0.05) * np.arange(n, dtype=np.float32), np.float32(-60.0)), None)
    out["ramp_down_up"] = (np.float32(-0.11) * (np.arange(n) % 97).astype(np.float32), None)
    for name in X.names(n):
        e = X.population(n, name)
        out["catalogue:" + name] = (e["logw"], e.get("max"))
    return out


def run_fill(eng, logw, m, frame, stamp, gate_frac=None):
    """quantise + scan, then the ancestors' launch with survivor marks -> (anc, mark) on the host; the slots behind n must stay
    as they were"""
    n = len(logw)
    if gate_frac is not None:
        eng.resample_gate_set(gate_frac)
    d_logw = torch.empty(n, device=DEV)
    eng.logweight_dev(None, dev(logw), 0.0, n, d_logw, None)
    d_max = None if m is None else dev(np.array([m], np.float32))
    eng.quantise_scan_dev(d_logw, d_max, n, None)
    anc = torch.full((n + GUARD,), -7, dtype=torch.int32, device=DEV)
    mark = torch.zeros(n + GUARD, dtype=torch.int32, device=DEV)
    so = SurvivorOut(mark.data_ptr(), stamp)
    rc = eng.lib.slam_ancestors_survivors_dev(eng.h, C.c_int(n), C.c_uint64(SEED), C.c_uint32(frame), C.c_void_p(anc.data_ptr()),
                                              C.byref(so))
    assert rc == 0
    torch.cuda.synchronize()
    anc, mark = anc.cpu().numpy(), mark.cpu().numpy()
    assert (anc[n:] == -7).all() and not mark[n:].any(), "stores behind the population"
    return anc[:n], mark[:n]


def check(eng, n, name, logw, m, frame):
    wq, _ = X.quantised(logw, m)
    want = X.exact_ancestors(wq, SEED, frame)[0]
    stamp = 11 + frame % 1000
    got, mark = run_fill(eng, logw, m, frame, stamp)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"n = {n}, {name}, frame {frame}: {bad.size} slots differ, the first: slot {bad[0]} got {got[bad[0]]} want {want[bad[0]]}"
    kept = np.zeros(n, bool)
    kept[want] = True
    assert np.array_equal(mark == stamp, kept) and not mark[~kept].any(), f"n = {n}, {name}, frame {frame}: survivor marks"
    return want


@pytest.mark.parametrize("n", SIZES)
def test_ancestors_and_marks_at_every_seam(engines, n):
    eng = engines[0]
    for name, (logw, m) in own_populations(n).items():
        for frame in FRAMES:
            want = check(eng, n, name, logw, m, frame)
            if name.startswith("only@"):
                assert (want == int(name[5:])).all()
        if name == "all_equal":
            assert np.array_equal(want, np.arange(n))
    # the binding without marks: the same launch
    logw, m = own_populations(n)["ramp_down_up"]
    d_logw = torch.empty(n, device=DEV)
    eng.logweight_dev(None, dev(logw), 0.0, n, d_logw, None)
    eng.quantise_scan_dev(d_logw, None, n, None)
    anc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.ancestors_from_scan_dev(n, SEED, 5, anc)
    torch.cuda.synchronize()
    assert np.array_equal(anc.cpu().numpy(), X.exact_ancestors(X.quantised(logw)[0], SEED, 5)[0])


def _mixed(n):
    """runs of every length: a saw of weights, 0 among them, and one particle with about a quarter of the slots"""
    lw = np.float32(-0.02) * (np.arange(n) % 1000).astype(np.float32)
    lw[3::17] = X.ZERO
    lw[n // 2 + 1] = np.float32(9.0)
    return lw


@pytest.mark.parametrize("n", [524288, 600000])
def test_ancestors_and_marks_at_the_top_of_one_turn_and_above(engines, n):
    """524 288: 256 tile totals, one per thread; 600 000: 293, a second turn of the loop over them"""
    want = check(engines[0], n, "mixed", _mixed(n), None, 5)
    assert np.bincount(want, minlength=n).max() > n // 8
    want = check(engines[0], n, f"only@{n // 2}", _carriers(n, [n // 2], [0.0]), None, 5)
    assert (want == n // 2).all()


@pytest.mark.parametrize("n", [65, 2049, 6149])
def test_a_gated_frame_that_keeps_its_population(engines, n):
    gated = engines[1]
    logw = np.full(n, X.CARRIER, np.float32)   # ESS = n: kept at every threshold
    for frame in FRAMES:
        got, mark = run_fill(gated, logw, None, frame, 3 + frame % 1000, gate_frac=0.5)
        assert not gated.resample_happened()
        assert np.array_equal(got, np.arange(n)) and (mark == 3 + frame % 1000).all()
    logw = _carriers(n, [n // 3], [0.0])        # ESS = 1: resamples, and the marks are the search's
    got, mark = run_fill(gated, logw, None, 5, 9, gate_frac=0.5)
    assert gated.resample_happened()
    assert (got == n // 3).all() and np.flatnonzero(mark).tolist() == [n // 3] and mark[n // 3] == 9
    gated.resample_gate_set(0.0)


def test_session_against_the_cpu_specification():
    """n = 4099, L = 261, split layout with survivor rows, six frames: poses, log-weights, ancestors and the map rows of every slot
    — read through the pending gather, no settle in between — are the bits of the CPU specification loop (the frame of
    tests/test_gpu_resample_populations.py), the ancestors those of the exact integers, and the distinct-ancestor estimate the
    launch hands the host lies in [1, n] (it steers speed, not results)."""
    import test_gpu_resample_populations as R

    S, w = R._session_world()
    n = S.N
    assert (n, S.L) == (4099, 261)
    poses = [p[:n] for p in w["poses"]]
    sessions = {"split, survivor rows": R._open(n, "split", True, poses)}
    cpu = R._spec_loop(n, poses)
    launches = {}
    for f in range(6):
        logw, anc = R._frame(sessions, cpu, w["fr"][f], n, launches)
        wq, _ = X.quantised(logw)
        assert np.array_equal(anc, X.exact_ancestors(wq, S.SEED, f)[0]), f"frame {f}"
    assert launches["split, survivor rows"] >= 2   # survivor frames really ran: the launch behind the resample, a settle per view
    eng = sessions["split, survivor rows"][0]
    eng.sync()
    heads, hn = eng.resample_heads()
    assert hn == n and 1 <= heads <= n, (heads, hn)
    R._close(sessions)
