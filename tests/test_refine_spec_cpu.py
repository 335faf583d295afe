"""The refinement specification (tests/_refine_spec.py) on the CPU: the properties the GPU kernel is
then held to bit for bit (tests/test_gpu_refine.py)."""
import numpy as np
import pytest

import _refine_spec as RS
from conftest import bits

STEPS = (0.05, 0.008727)


@pytest.fixture(scope="module")
def room(orc):
    return RS.make_room(orc)


def test_no_pose_moves_on_an_all_free_grid(orc):
    """Every cell at the cap and every beam of every candidate well inside the grid (or, for the first five poses, every
    beam outside): all 27 candidates tie, and the incumbent rule keeps the centre (FastMatch's start from +inf would walk
    to candidate 0)."""
    rows = cols = 64
    meta = orc.meta(rows, cols, cols, 0.1, -3.2, -3.2)
    edt = np.full((rows, cols), 10.0, np.float32)
    rng = np.random.default_rng(3)
    bx, by = (rng.uniform(-1.2, 1.2, 40).astype(np.float32) for _ in range(2))   # |rotated beam| <= 1.7 m, pose and
    x, y, th = (rng.uniform(-0.5, 0.5, 50).astype(np.float32) for _ in range(3))   # lattice <= 0.75 m: cells 7 .. 57 of 64
    x[:5] = 50.0   # entirely outside as well
    for sweeps in (1, 2, 5, 16):
        rx, ry, rt, sc, cn = RS.refine(orc, meta, edt, bx, by, x, y, th, *STEPS, sweeps)
        assert np.array_equal(bits(rx), bits(x)) and np.array_equal(bits(ry), bits(y)) and np.array_equal(bits(rt), bits(th))
        s0, c0 = orc.score_poses_det(meta, edt, bx, by, x, y, th)
        assert np.array_equal(bits(sc), bits(s0)) and np.array_equal(cn, c0)


def test_zero_steps_return_the_score_unchanged(orc, room):
    meta, edt, bx, by = room
    rng = np.random.default_rng(4)
    x, y, th = (rng.uniform(-0.5, 0.5, 30).astype(np.float32) for _ in range(3))
    rx, ry, rt, sc, cn = RS.refine(orc, meta, edt, bx, by, x, y, th, 0.0, 0.0, 3)
    s0, c0 = orc.score_poses_det(meta, edt, bx, by, x, y, th)
    assert np.array_equal(bits(rx), bits(x)) and np.array_equal(bits(ry), bits(y)) and np.array_equal(bits(rt), bits(th))
    assert np.array_equal(bits(sc), bits(s0)) and np.array_equal(cn, c0)


def test_displaced_poses_descend_monotonically_to_a_fixed_point(orc, room):
    """Poses one and two lattice steps away from the scan's true pose (the origin, so that start -/+ step is exact): the
    score never rises from sweep to sweep; a pose ONE step away has the true pose in its first lattice, so it ends no higher
    than the true pose's score; a pose TWO steps away has the midpoint — a neighbour of the true pose — in its first lattice,
    so it ends no higher than the midpoint's score; and one more sweep on a pose whose centre won changes nothing."""
    meta, edt, bx, by = room
    t, r = (np.float32(v) for v in STEPS)
    unit = np.array([(1, 0, 0), (0, 1, 0), (0, 0, 1), (-1, 0, 0), (0, -1, 0), (0, 0, -1), (1, 1, 0), (1, -1, 1), (-1, 1, -1)], np.float32)
    for k in (1, 2):
        d = unit * np.float32(k)
        x, y, th = d[:, 0] * t, d[:, 1] * t, d[:, 2] * r
        bound_pose = unit * np.float32(k - 1)   # k = 1: the true pose; k = 2: the midpoint
        bound, _ = orc.score_poses_det(meta, edt, bx, by, bound_pose[:, 0] * t, bound_pose[:, 1] * t, bound_pose[:, 2] * r)
        start, _ = orc.score_poses_det(meta, edt, bx, by, x, y, th)
        hist = []
        out = RS.refine(orc, meta, edt, bx, by, x, y, th, t, r, 8, history=hist)
        prev = start
        for h in hist:
            assert np.all(h[3] <= prev)
            prev = h[3]
        assert np.all(out[3] <= bound)
        # the score reported is the score of the pose reported
        s_end, c_end = orc.score_poses_det(meta, edt, bx, by, out[0], out[1], out[2])
        assert np.array_equal(bits(s_end), bits(out[3])) and np.array_equal(c_end, out[4])
        # fixed point: wherever the centre won, later sweeps kept the pose
        for a, b in zip(hist, hist[1:]):
            stay = a[5] == 13
            assert np.all(b[5][stay] == 13)
            for q in range(4):
                assert np.array_equal(bits(a[q][stay]), bits(b[q][stay]))
        assert np.all(hist[-1][5] == 13), "8 sweeps did not reach a fixed point two steps from the true pose"
        again = RS.refine(orc, meta, edt, bx, by, out[0], out[1], out[2], t, r, 1)
        for q in range(4):
            assert np.array_equal(bits(again[q]), bits(out[q]))


def test_the_binding_declares_the_new_entry_points():
    from __graft_entry__ import load_package

    sig = load_package().SIGNATURES
    for name in ("slam_refine_poses_dev", "slam_motion_refine_dev", "slam_pf_refine_set"):
        assert name in sig
