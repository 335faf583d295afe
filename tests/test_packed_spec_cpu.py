"""tests/_packed_spec.py on the CPU oracle's capped EDTs (oracle.edt, "window"): which grids pack, fixed here before the GPU
tests (tests/test_gpu_packed_grid.py) hold the engine to the same verdicts on the same grids.  Needs no GPU.

Why cap 16.0 still packs: its distances below the cap are sqrtf(d2) with d2 <= 255, 255 = 3 * 5 * 17 is no sum of two squares
(nor are 251 .. 254: 250 = 15^2 + 5^2 = 13^2 + 9^2 is the largest below 256), and 16.0 itself is the grid's top value.  Above
16.0 a grid may hold 16.0 = sqrtf(256), sqrtf(257) ... beside the cap: more than one value that is no sqrtf(0 .. 254).
"""
import numpy as np
import pytest

import _packed_spec as PS
from conftest import bits


def test_the_roots_are_correctly_rounded_float32():
    """np.sqrt on float32 against the square root of the exact integer in float64, rounded once (the double rounding is
    innocuous for a 24-bit result of a 53-bit one: Figueroa), and the properties the statement leans on"""
    want = np.sqrt(np.arange(255, dtype=np.float64)).astype(np.float32)
    assert PS.ROOTS.dtype == np.float32 and np.array_equal(bits(PS.ROOTS), bits(want))
    assert np.all(np.diff(PS.ROOTS) > 0) and PS.ROOTS[0] == 0 and PS.ROOTS[225] == 15
    sums = {a * a + b * b for a in range(17) for b in range(17)}
    assert 250 in sums and 256 in sums and not sums & {251, 252, 253, 254, 255}


@pytest.mark.parametrize("case", sorted(PS.cap_cases()), ids=lambda c: f"{c[0]}-{c[1]}-cap{c[2]}")
def test_capped_edts(case):
    shape, kind, cap = case
    rows, cols, ld = PS.shape_of(shape)
    assert rows % 8 and cols % 16 and ld > cols
    occ, edt = PS.edt_case(shape, kind, cap)
    want = PS.cap_cases()[case]
    assert PS.packs(edt, rows, cols) == want
    cells = edt[:rows, :cols]
    top = PS.top_value(edt, rows, cols)
    assert cells.min() == 0 and top <= np.float32(cap) and np.all(edt[:, cols:] == -1)
    reaches_cap = top == np.float32(cap)
    if kind in ("sparse", "single"):
        assert reaches_cap, "a cell at the cap was meant"
    if kind == "sparse" and cap >= 15.9:
        # the end of the code range: d2 = 250 needs cap^2 > 250 (15.9^2 = 252.8)
        assert PS.largest_root(edt, rows, cols) == 250
    if cap in PS.CAPS_ABOVE and kind == "single":
        assert np.count_nonzero(np.unique(cells) >= 16) >= 3, "16.0, something between and the cap were meant"
    if cap in PS.CAPS_ABOVE and kind == "dense":
        # nothing reaches the cap: the top value is the square root of an integer itself
        assert not reaches_cap and np.float32(top).view(np.uint32) in PS.ROOT_BITS
    if cap == 0.0:
        assert not cells.any()
    if cap == 0.5:
        assert set(np.unique(cells)) == {np.float32(0), np.float32(0.5)}
    if cap == 3.5 and kind == "sparse":
        assert PS.largest_root(edt, rows, cols) == 10 and top == np.float32(3.5)   # 10 = 9 + 1 < 12.25 <= 13 = 9 + 4


def test_no_cell_reaches_the_cap_at_the_usual_cap_either():
    rows, cols, ld = PS.shape_of("23x37")
    _, edt = PS.edt_case("23x37", "dense", 10.0)
    assert PS.top_value(edt, rows, cols) < 10 and PS.packs(edt, rows, cols)


@pytest.mark.parametrize("shape", sorted(PS.SHAPES) + sorted(PS.TOO_SMALL))
def test_every_shape_s_usual_grid_packs_and_its_scaled_copy_does_not(shape):
    rows, cols, ld = PS.shape_of(shape)
    _, edt = PS.edt_case(shape, "sparse", 10.0)
    assert PS.packs(edt, rows, cols)
    scaled = PS.scaled_case(shape, "sparse", 10.0)
    assert not PS.packs(scaled, rows, cols)
    small = shape in PS.TOO_SMALL
    assert PS.engine_state(edt, rows, cols, 3072) == (0 if small else 1)
    assert PS.engine_state(scaled, rows, cols, 131072) == (0 if small else 2)
    assert PS.engine_state(edt, rows, cols, 3071) == 0


def test_what_else_does_not_pack():
    g = np.zeros((8, 16), np.float32)
    assert PS.packs(g, 8, 16)
    g[3, 4] = 7.25                       # the top value may be anything ...
    assert PS.packs(g, 8, 16)
    g[0, 0] = np.sqrt(np.float32(254))   # ... but it is the LARGEST cell: 7.25 no longer is, and is no root
    assert not PS.packs(g, 8, 16)
    g[3, 4] = np.sqrt(np.float32(255))   # the top value again
    assert PS.packs(g, 8, 16)
    g[5, 5] = 16.0                       # 16.0 is the top now, and sqrtf(255) is no root of 0 .. 254
    assert not PS.packs(g, 8, 16)
    g[3, 4] = 15.0
    assert PS.packs(g, 8, 16)
    h = np.zeros((8, 16), np.float32)
    h[1, 1] = np.nextafter(np.float32(3), np.float32(4))   # one ulp beside sqrtf(9), under a larger top
    h[2, 2] = 5
    assert not PS.packs(h, 8, 16)
    h[1, 1] = np.nan
    assert not PS.packs(h, 8, 16)
    h[1, 1] = -1
    assert not PS.packs(h, 8, 16)
    # cells outside the rows x cols rectangle do not count
    wide = np.full((9, 20), -3.0, np.float32)
    wide[:8, :16] = 2
    assert PS.packs(wide, 8, 16) and not PS.packs(wide, 9, 16)
