"""slam_pose_modes_dev — the modes of a pose population — against its exact restatement (tests/_modes_spec.py, pinned by
tests/test_modes_spec_cpu.py): every field of every mode, the counts and the statuses, bit for bit; every case a second time on the
permuted population.  The session form: tests/test_gpu_modes_session.py."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _estimate_spec as E
import _modes_spec as M
import _spread_spec as S
from __graft_entry__ import load_package

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELL, H, MM = 0.5, 8, 4
# one particle, a wavefront and its neighbours, more than one workgroup, several persistent workgroups, one past a round grid
SIZES = [1, 63, 64, 65, 257, 4097, 65537]
INVALID_ARG, CAPACITY = -2, -5


@pytest.fixture(scope="module")
def rig():
    pkg = load_package()
    eng = pkg.Engine(0)
    yield SimpleNamespace(pkg=pkg, eng=eng)
    eng.close()


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _call(rig, x, y, th, ref, idx=None, carry=None, cell=CELL, hbins=H, max_modes=MM):
    d = _dev(x, y, th, None if idx is None else np.asarray(idx, np.int32), carry)
    torch.cuda.synchronize()
    modes, cells, wt = rig.eng.pose_modes_dev(d[0], d[1], d[2], len(x), ref, cell, hbins, max_modes, d_idx=d[3], d_carry=d[4])
    return M.Result([M.Mode(m["pose"], m["mass"], m["cell"], m["ncells"], m["weight"]) for m in modes], cells, wt)


def _weights(n, seed):
    logw = np.random.default_rng(seed).normal(-3.0, 1.5, n).astype(np.float32)
    logw[::7] = -200.0                                   # some particles without any weight: they make no cell
    w16, _ = M.weights16(logw)
    return w16, E.oracle.weight_carry(logw, np.float32(np.fmax.reduce(logw)))


def _check(rig, pop, ref=0.3, tag="", **kw):
    """plain, gathered, weighted and both, each also on the permuted population -> the plain result"""
    x, y, th = pop
    n = len(x)
    rng = np.random.default_rng(n + 1)
    idx = rng.integers(0, n, n)
    w16, carry = _weights(n, n)
    p = rng.permutation(n)
    first = None
    for form, use_idx, use_w in (("plain", False, False), ("gathered", True, False), ("weighted", False, True), ("both", True, True)):
        want = M.modes_spec(x, y, th, idx if use_idx else None, ref, kw.get("cell", CELL), kw.get("hbins", H), kw.get("max_modes", MM),
                            w16 if use_w else None)
        got = _call(rig, x, y, th, ref, idx if use_idx else None, carry if use_w else None, **kw)
        assert M.same(got, want), (tag, form, n, got, want)
        if use_idx:     # the same multiset of particles behind another gather, the weights travelling with their slots
            got_p = _call(rig, x, y, th, ref, idx[p], carry[p] if use_w else None, **kw)
        else:
            got_p = _call(rig, x[p], y[p], th[p], ref, None, carry[p] if use_w else None, **kw)
        assert M.same(got_p, want), (tag, form, "permuted", n, got_p, want)
        first = first or got
    return first


POPULATIONS = {
    "identical": lambda n: S.spread_population("identical", n),
    "two_clusters": lambda n: S.spread_population("two_clusters", n),
    "straddle_zero": lambda n: M.modes_population("straddle_zero", n, CELL),
    "heading_wrap": lambda n: M.modes_population("heading_wrap", n, CELL),
    "far_cloud": lambda n: S.spread_population("far_cloud", n),
}


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", sorted(POPULATIONS))
def test_populations_at_every_seam(rig, name, n):
    got = _check(rig, POPULATIONS[name](n), tag=name)
    if name == "identical":
        assert got.cells == 1 and len(got.modes) == 1 and got.modes[0].weight == n and got.modes[0].mass == np.float32(1.0)
    if name == "two_clusters" and n > 1:
        assert len(got.modes) == 2
    if name in ("straddle_zero", "heading_wrap") and n >= 63:
        assert len(got.modes) == 1 and got.modes[0].ncells > 1 and got.modes[0].weight == n


def test_scatter_loads_the_table_and_spills_lds(rig):
    """some 20 000 distinct cells: far more per workgroup than its LDS table holds"""
    pop = M.modes_population("scatter", 65537, CELL)
    got = _check(rig, pop, tag="scatter", hbins=16, max_modes=8)
    assert 15000 < got.cells <= 40000 and len(got.modes) == 8, got.cells


@pytest.mark.parametrize("name,keys", [("wave_64_keys", 64), ("wave_2_keys", 2)])
def test_distinct_keys_per_wavefront(rig, name, keys):
    """every wavefront holds exactly 64 distinct keys, or exactly 2: the serve-one-key-at-a-time loop at both ends"""
    n = 4096 + 64
    pop = M.modes_population(name, n, CELL)
    ix, iy, b, *_ = M.particle_terms(*pop, None, 0.3, CELL, H)
    for w in range(0, n, 64):
        assert len(set(zip(ix[w:w + 64].tolist(), iy[w:w + 64].tolist(), b[w:w + 64].tolist()))) == keys
    x, y, th = pop
    want = M.modes_spec(x, y, th, None, 0.3, CELL, H, 8)
    got = _call(rig, x, y, th, 0.3, max_modes=8)
    assert M.same(got, want) and got.cells == keys and len(got.modes) == min(keys, 8), (got, want)
    w16, carry = _weights(n, 3)
    assert M.same(_call(rig, x, y, th, 0.3, carry=carry, max_modes=8), M.modes_spec(x, y, th, None, 0.3, CELL, H, 8, w16))


def test_one_heading_bin_and_sixty_four(rig):
    pop = S.spread_population("two_clusters", 4097)
    for hb in (1, 4, 64):
        _check(rig, pop, tag=f"hbins {hb}", hbins=hb)


def test_second_call_owes_nothing_to_the_first(rig):
    a, b = M.modes_population("scatter", 4097, CELL), S.spread_population("two_clusters", 257)
    for pop in (a, b, a, b):
        assert M.same(_call(rig, *pop, 0.1), M.modes_spec(*pop, None, 0.1, CELL, H, MM))


def test_no_weight_at_all_is_the_plain_form(rig):
    x, y, th = S.spread_population("two_clusters", 257)
    carry = np.full(257, -200.0, np.float32)
    assert M.same(_call(rig, x, y, th, 0.1, carry=carry), M.modes_spec(x, y, th, None, 0.1, CELL, H, MM))


def _refused(rig, status, *args, **kw):
    with pytest.raises(rig.pkg.SlamError) as err:
        _call(rig, *args, **kw)
    assert err.value.status == status, str(err.value)
    return str(err.value)


def test_refusals_leave_the_engine_sound(rig):
    good = S.spread_population("two_clusters", 4097)
    want = M.modes_spec(*good, None, 0.1, CELL, H, MM)
    # capacity: 65 537 particles at x = i * cell; 65 536 are accepted
    x = (np.arange(M.MAX_CELLS + 1) * CELL).astype(np.float32)
    y, th = np.zeros_like(x), np.zeros_like(x)
    assert "65536" in _refused(rig, CAPACITY, x, y, th, 0.0)
    assert M.same(_call(rig, *good, 0.1), want)
    full = _call(rig, x[:-1], y[:-1], th[:-1], 0.0)
    assert M.same(full, M.modes_spec(x[:-1], y[:-1], th[:-1], None, 0.0, CELL, H, MM)) and full.cells == M.MAX_CELLS
    # domain: one particle at u = 2^20, one NaN heading
    for axis, value in ((0, np.float32(2.0 ** 20 * CELL)), (2, np.float32(np.nan))):
        bad = [a.copy() for a in good]
        bad[axis][1234] = value
        with pytest.raises(M.OutOfDomain):
            M.modes_spec(*bad, None, 0.1, CELL, H, MM)
        assert "1 particles" in _refused(rig, INVALID_ARG, *bad, 0.1)
        assert M.same(_call(rig, *good, 0.1), want)
    inside = [a.copy() for a in good]
    inside[0][1234] = np.nextafter(np.float32(2.0 ** 20 * CELL), np.float32(0.0))
    assert M.same(_call(rig, *inside, 0.1), M.modes_spec(*inside, None, 0.1, CELL, H, MM))


def test_refusals_do_not_write_the_outputs(rig):
    import ctypes as C
    pkg, eng = rig.pkg, rig.eng
    x = (np.arange(M.MAX_CELLS + 1) * CELL).astype(np.float32)
    bad = [a.copy() for a in S.spread_population("two_clusters", 257)]
    bad[2][5] = np.nan
    for pop, status in (((x, np.zeros_like(x), np.zeros_like(x)), CAPACITY), (bad, INVALID_ARG)):
        d = _dev(*pop)
        modes = (pkg.PfMode * pkg.MAX_MODES)()
        C.memset(modes, 0x5A, C.sizeof(modes))
        nm, cells, wt = C.c_int(-7), C.c_int(-8), C.c_int64(-9)
        rc = eng.lib.slam_pose_modes_dev(eng.h, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, None, len(pop[0]), 0.0, CELL, H, MM,
                                         modes, C.byref(nm), C.byref(cells), C.byref(wt))
        assert rc == status and (nm.value, cells.value, wt.value) == (-7, -8, -9)
        assert bytes(modes) == b"\x5a" * C.sizeof(modes)


@pytest.mark.parametrize("kw", [dict(hbins=2), dict(hbins=3), dict(hbins=65), dict(hbins=0), dict(max_modes=0), dict(max_modes=9),
                                dict(cell=0.0), dict(cell=-1.0), dict(cell=float("inf")), dict(cell=float("nan"))])
def test_bad_parameters(rig, kw):
    _refused(rig, INVALID_ARG, *S.spread_population("two_clusters", 65), 0.1, **kw)


def test_negative_n(rig):
    d = _dev(*S.spread_population("two_clusters", 65))
    for n in (-1, 0):
        with pytest.raises(rig.pkg.SlamError) as err:
            rig.eng.pose_modes_dev(d[0], d[1], d[2], n, 0.1, CELL, H, MM)
        assert err.value.status == INVALID_ARG
