"""When does a grid pack?  The statement of include/slam_hip.h (slam_grid_set_dev, slam_grid_packed_state) in numpy, and the
grids the CPU test and the GPU tests share.  TEST INFRASTRUCTURE for test_packed_spec_cpu.py and test_gpu_packed_grid.py.

The many-pose scorers may read a one-byte-per-cell copy of a grid: 255 codes stand for sqrtf(0) .. sqrtf(254), the 256th for
the grid's largest value.  Said of the grid's CONTENTS alone, without the codes:

  a float32 grid packs  iff  every cell of its rows x cols rectangle is, as a bit pattern, the correctly rounded sqrtf(k) of an
  integer k in 0 .. 254, or the grid's top value (its largest cell; any one bit pattern).

Everything here is float32: np.sqrt of a float32 array is the correctly rounded binary32 square root.  The grids in question
hold distances: no negative cell, no NaN (such a grid is said not to pack; no test feeds one to the engine).

engine_state() adds what the header says of the engine beyond the contents: a verdict exists only once a scorer of at least
3 072 poses has read the grid, and never for a grid under 8 rows or 16 columns.
"""
import functools

import numpy as np

MIN_POSES, MIN_ROWS, MIN_COLS = 3072, 8, 16   # include/slam_hip.h: slam_grid_set_dev / slam_grid_packed_state

ROOTS = np.sqrt(np.arange(255, dtype=np.float32))   # sqrtf(0) .. sqrtf(254), float32 in, float32 out
assert ROOTS.dtype == np.float32
ROOT_BITS = ROOTS.view(np.uint32)


def _cells(grid, rows, cols):
    g = np.asarray(grid)
    assert g.dtype == np.float32 and g.ndim == 2 and g.shape[0] >= rows and g.shape[1] >= cols
    return np.ascontiguousarray(g[:rows, :cols])


def top_value(grid, rows, cols):
    """the grid's largest cell (float32)"""
    return _cells(grid, rows, cols).max()


def packs(grid, rows, cols) -> bool:
    c = _cells(grid, rows, cols)
    if c.size == 0 or np.isnan(c).any() or np.signbit(c).any():
        return False
    patterns = np.unique(c.view(np.uint32))
    top = np.float32(c.max()).view(np.uint32)
    others = patterns[patterns != top]
    return bool(np.isin(others, ROOT_BITS).all())


def largest_root(grid, rows, cols, below_top=True):
    """the largest k in 0 .. 254 whose sqrtf(k) is a cell of the grid (with below_top: of the cells other than the top value);
    -1: none"""
    c = _cells(grid, rows, cols)
    b = c.view(np.uint32)
    if below_top:
        b = b[b != np.float32(c.max()).view(np.uint32)]
    k = np.flatnonzero(np.isin(ROOT_BITS, b))
    return int(k[-1]) if k.size else -1


def engine_state(grid, rows, cols, most_poses):
    """slam_grid_packed_state of a grid whose largest scorer call since it last changed had `most_poses` poses"""
    if most_poses < MIN_POSES or rows < MIN_ROWS or cols < MIN_COLS:
        return 0
    return 1 if packs(grid, rows, cols) else 2


# ------------------------------------------------------------------ the shared grids
# (rows, cols, ld): the smallest that packs; one over in both; rows % 8, cols % 16 != 0 with ld > cols; the workload's smoke
# shape; tall and thin (one strip of 16 columns, 257 rows: 33 patches of 8 rows, the last with one)
SHAPES = {"8x16": (8, 16, 16), "9x17": (9, 17, 17), "23x37": (23, 37, 41), "150x190": (150, 190, 200), "257x16": (257, 16, 16)}
TOO_SMALL = {"7x64": (7, 64, 64), "64x15": (64, 15, 15)}   # one row / one column short of a packed copy
CAPS = (0.0, 0.5, 1.0, 3.5, 10.0, 15.0, 15.9, 15.96, 16.0)
CAPS_ABOVE = (16.5, 17.0, 32.0)
CAP_SHAPES = ("23x37", "150x190")
PIXEL = 0.1


def shape_of(name):
    return SHAPES[name] if name in SHAPES else TOO_SMALL[name]


def occupancy(shape, kind, seed=0):
    """int32 [rows][ld].  single: cell (0, 0) alone.  sparse: cell (0, 0) and, per 8 000 cells, about one more at random — free
    cells up to sqrt(250) and farther from all of them.  dense: three cells in ten.  empty: none.  The padding columns
    (ld > cols) are occupied throughout: nothing may read them."""
    rows, cols, ld = shape_of(shape)
    rng = np.random.default_rng(1000 + seed)
    occ = np.zeros((rows, ld), np.int32)
    if kind in ("single", "sparse"):
        occ[0, 0] = 1
    if kind == "sparse":
        occ[:, :cols] |= rng.random((rows, cols)) < 1.0 / 8000
    elif kind == "dense":
        occ[:, :cols] = rng.random((rows, cols)) < 0.3
    else:
        assert kind in ("single", "empty"), kind
    occ[:, cols:] = 1
    return occ


@functools.lru_cache(maxsize=None)
def edt_case(shape, kind, cap, seed=0):
    """-> (occ, the CPU oracle's capped EDT of it [rows][ld] with the padding columns at -1, read-only); made once"""
    import oracle

    oracle.build(ref=False)
    rows, cols, ld = shape_of(shape)
    occ = occupancy(shape, kind, seed)
    edt = np.full((rows, ld), -1.0, np.float32)
    oracle.edt(occ, rows, cols, cap, "window", out=edt)
    occ.setflags(write=False)
    edt.setflags(write=False)
    return occ, edt


@functools.lru_cache(maxsize=None)
def scaled_case(shape, kind, cap, seed=0):
    """the existing suites' "float" grid: every cell of the EDT times a random factor in [0.9, 1.1]"""
    rows, cols, ld = shape_of(shape)
    _, edt = edt_case(shape, kind, cap, seed)
    out = (edt * np.random.default_rng(9).uniform(0.9, 1.1, edt.shape)).astype(np.float32)
    out.setflags(write=False)
    return out


# every case of a capped EDT the tests run: (shape, occupancy, cap) -> does it pack?  Fixed here, by reasoning on distances (a
# capped EDT holds 0, sqrtf(d2) for integer d2 < cap^2, and the cap), and checked against packs() on the CPU before a GPU sees it.
def cap_cases():
    cases = {}
    for shape in CAP_SHAPES:
        for kind in ("sparse", "dense"):
            for cap in CAPS:   # cap <= 16: d2 < 256, and 255 is no sum of two squares: d2 <= 254 (in fact <= 250)
                cases[(shape, kind, cap)] = True
    for cap in CAPS_ABOVE:     # one occupied corner: cells at 16.0 (d2 = 256), at sqrtf(257) ... and at the cap
        cases[("23x37", "single", cap)] = False
        cases[("150x190", "single", cap)] = False
    cases[("23x37", "dense", 17.0)] = True    # three cells in ten occupied: nothing is 16 cells from all of them
    cases[("150x190", "dense", 17.0)] = True
    cases[("23x37", "dense", 32.0)] = True
    return cases
