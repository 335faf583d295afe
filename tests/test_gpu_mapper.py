"""The mapper's device stages — clean_scan, transform, crop, rasterise, map_append and the chained FastMatch pair — against the
frame loop restated in the oracle's stage functions (tests/_mapper_spec.py), bit for bit, after every frame, through
``slam_mapper_device_view``.  The cases and what each of them exercises are pinned on the CPU by
tests/test_mapper_spec_cpu.py; the existing end-to-end runs only ever see the pose and the final map."""
import ctypes as C

import numpy as np
import pytest

import _mapper_spec as ms
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu

SLAM_ERR_CAPACITY = -5


@pytest.fixture(scope="module")
def pkg():
    return load_package()


@pytest.fixture(scope="module")
def eng(pkg):
    e = pkg.Engine(0)
    yield e
    e.close()


def host(a):
    import torch

    return torch.as_tensor(a, device="cuda").cpu().numpy()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} != {want.shape}"
    g = got.view(np.uint32) if got.dtype == np.float32 else got
    w = want.view(np.uint32) if want.dtype == np.float32 else want
    if not np.array_equal(g, w):
        bad = np.argwhere(g != w)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {g.size} differ, first at {i}: got {got[i]!r}, want {want[i]!r}")


def meta_words(m):
    return np.frombuffer(bytes(m), np.int32)


def check(eng, mp, spec, what):
    """The mapper's whole state after a frame against the spec's."""
    eng.sync()
    v = mp.view()
    nscan, msize, lsize = (int(c) for c in host(v["counts"]))
    assert nscan == spec.scan_n, f"{what}: nscan {nscan} != {spec.scan_n}"
    same(host(v["bx"])[:nscan], spec.sx, f"{what}: bx")
    same(host(v["by"])[:nscan], spec.sy, f"{what}: by")
    if spec.made_world:
        same(host(v["tx"])[:nscan], spec.tx, f"{what}: tx")
        same(host(v["ty"])[:nscan], spec.ty, f"{what}: ty")
    assert msize == spec.map_n, f"{what}: msize {msize} != {spec.map_n}"
    same(host(v["mx"])[:msize], spec.map_x, f"{what}: mx")
    same(host(v["my"])[:msize], spec.map_y, f"{what}: my")
    if spec.rebuilt:
        assert lsize == len(spec.lx), f"{what}: lsize {lsize} != {len(spec.lx)}"
        same(host(v["lx"])[:lsize], spec.lx, f"{what}: lx")
        same(host(v["ly"])[:lsize], spec.ly, f"{what}: ly")
        meta = host(v["meta"])
        for k in (0, 1):
            same(meta[k], meta_words(spec.meta[k]), f"{what}: meta[{k}] (rows, cols, ld, pixel, min_x, min_y)")
            assert v["ld"][k] == ms.LD[k]
            same(host(v["occ"][k]), spec.occ[k], f"{what}: occupancy grid {k}, whole storage")
            r, c = spec.meta[k].rows, spec.meta[k].cols
            same(host(v["edt"][k])[:r, :c], spec.edt[k][:r, :c], f"{what}: EDT {k}")
    same(v["pose"], spec.pose, f"{what}: pose")
    same(v["prev"], spec.prev, f"{what}: prev")
    same(v["map_pose"], spec.map_pose, f"{what}: map_pose")
    assert v["mini_updated"] == spec.mini_updated, f"{what}: mini_updated"
    assert v["frame"] == spec.frame, f"{what}: frame"
    assert v["nhits"] == spec.hits_n, f"{what}: hit count {v['nhits']} != {spec.hits_n}"
    # the scratch is zeroed by first_frame and persists from then on: all of it is defined, not only the prefix
    # [0, largest count of any candidate) the last call wrote
    same(host(v["hits"]), spec.hits[: spec.nbeams], f"{what}: hit scratch")


def run(orc, pkg, eng, name, mp=None, frames=None):
    """The case on a mapper (a fresh one unless given) against a fresh spec, compared after every frame; -> (mapper, poses)."""
    c = ms.case(orc, name)
    spec = c.spec(orc)
    if mp is None:
        mp = pkg.Mapper(eng, c.nbeams, c.angle_min, c.angle_inc, c.pkg_params(pkg) if c.changes else None)
    poses = []
    try:
        for f, r in enumerate(c.frames if frames is None else frames):
            if f == 0:
                mp.first_frame(r)
                spec.first_frame(r)
            else:
                pose = mp.next_frame(r)
                same(pose, spec.next_frame(r), f"{name} frame {f}: returned pose")
                poses.append(pose)
            check(eng, mp, spec, f"{name} frame {f}")
    except BaseException:
        mp.close()
        raise
    return mp, poses


@pytest.mark.parametrize("name", ms.ALL_CASES)
def test_every_stage_equals_the_spec(orc, pkg, eng, name):
    mp, _ = run(orc, pkg, eng, name)
    mp.close()


def test_201_columns_are_refused_and_the_engine_goes_on(orc, pkg, eng):
    """rasterise_kernel writes its meta record and clears its own ld x ld storage, then returns before the first point store
    when the grid does not fit; rebuild_grids reads the meta back and returns SLAM_ERR_CAPACITY before any EDT launch."""
    c = ms.case(orc, "raster-201")
    mp = pkg.Mapper(eng, c.nbeams, c.angle_min, c.angle_inc)
    try:
        mp.first_frame(c.frames[0])
        with pytest.raises(pkg.SlamError) as err:
            mp.next_frame(c.frames[1])
        assert err.value.status == SLAM_ERR_CAPACITY
    finally:
        mp.close()
    mp, _ = run(orc, pkg, eng, "raster-200")
    mp.close()


def test_second_first_frame_starts_over(orc, pkg, eng):
    mp, first = run(orc, pkg, eng, "restart")
    n1, x1, y1 = mp.map()
    mp, second = run(orc, pkg, eng, "restart", mp=mp)
    n2, x2, y2 = mp.map()
    mp.close()
    assert len(first) == len(second) == 4
    same(np.stack(second), np.stack(first), "poses of the second pass")
    assert n1 == n2
    same(x2, x1, "map x of the second pass")
    same(y2, y1, "map y of the second pass")


def test_get_map_respects_capacity_and_null_arrays(orc, pkg, eng):
    mp, _ = run(orc, pkg, eng, "restart")
    try:
        n, x, y = mp.map()
        assert n == len(x) == len(y) > 16
        assert mp.map(want_points=False) == (n, None, None)   # NULL arrays: the size comes back
        cap = n - 7
        n_cap, xc, yc = mp.map(capacity=cap)
        assert n_cap == n and len(xc) == cap
        same(xc, x[:cap], "map x with capacity below the size")
        same(yc, y[:cap], "map y with capacity below the size")
        # only `capacity` points are written
        gx, gy = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
        got = C.c_int32(-1)
        rc = eng.lib.slam_mapper_get_map_host(mp.h, gx.ctypes.data_as(C.c_void_p), gy.ctypes.data_as(C.c_void_p), cap, C.byref(got))
        assert rc == 0 and got.value == n
        same(gx[:cap], x[:cap], "x")
        same(gy[:cap], y[:cap], "y")
        assert np.isnan(gx[cap:]).all() and np.isnan(gy[cap:]).all()
        one = np.full(1, np.nan, np.float32)
        rc = eng.lib.slam_mapper_get_map_host(mp.h, one.ctypes.data_as(C.c_void_p), None, 1, C.byref(got))
        assert rc == 0 and got.value == n and np.isnan(one).all()   # one array NULL: nothing is written
    finally:
        mp.close()
