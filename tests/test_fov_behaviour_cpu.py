"""The field of view of the evidence stage (tests/_fov_spec.py) as a rule: a drive with the reference's own sensor — 1079 beams
over 269.5 degrees, a blind quarter behind the robot — past a pole that drifts into the blind quarter.  The chain detector (wrap =
0) -> association -> update -> evidence on the spec loops, in a box room with five poles.  Without the field of view the landmark
of pole 0 takes a miss in every frame it is behind the robot and is pruned, with line of sight or without (the blind bins are
empty: nothing is hidden there); with it the landmark keeps its slot and its evidence.  And on a drive where no pole leaves the arc
the bits are the same as without the field of view.  No GPU."""
import numpy as np
import pytest

import _detect_spec as D
import _fov_spec as V

F = np.float32
ANGLES = -2.351831 + 0.004363 * np.arange(1079)
EDGE = 0.1
RHO, HALF = 0.1, 6.0
POLES = np.array([(-1.5, 2), (3, -2), (4, .6), (1, 3.5), (2.5, 3)], np.float64)
FRONT_POLES = np.array([(-1, 3.5), (3, -2), (4, .6), (1, 3.5), (2.5, 3)], np.float64)   # no pole leaves the arc
N, SLOTS, FRAMES = 64, 8, 40
DP = (0.0, 0.03, 0.0)
KW = dict(seed=5, sigma=(0.005, 0.005, 0.001), meas_var=2.5e-3, score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 8, 9.0)
SIGHT = (128, 0.3)
RECORDED = tuple(range(0, FRAMES, 3))
# the bounds a session computes, with float64 cosine and sine: lo = bound(angle_min + edge), hi = bound(angle_max - edge)
FOV = (V.bound(F(ANGLES[0]) + F(EDGE)), V.bound(F(ANGLES[-1]) - F(EDGE)))


def scans_of(poles):
    return [D.raycast((0.0, 0.03 * (f + 1), 0.0), poles, RHO, HALF, noise=np.random.default_rng(100 + f), angles=ANGLES)[:2]
            for f in range(FRAMES)]


def drive(poles, fov, sight):
    world = dict(x=np.zeros(N, F), y=np.zeros(N, F), th=np.zeros(N, F), mp=np.zeros((N, 5, SLOTS), F))
    world["mp"][:, 2] = -1.0
    return V.frame_loop(world, scans_of(poles), N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, fov=fov, sight=sight,
                        score=False, detect_params=dict(wrap=0), **KW)


def landmark_of(fr, pole):
    """The evidence of the landmark of the frame's heaviest particle within 0.3 m of the pole's centre, None: there is none."""
    k = int(np.flatnonzero(fr["anc"] == np.argmax(fr["logw"]))[0])
    row, ev = fr["map"][k], fr["ev"][k]
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen] - pole[0], row[1, seen] - pole[1])
    near = seen[d <= 0.3]
    return int(ev[near[0]]) if len(near) else None


def test_the_bounds_wrap_round_the_blind_quarter():
    lo, hi = FOV
    assert lo.dtype == np.float32 and 2.0 < lo < 3.0 and 1.0 < hi < 2.0 and lo > hi   # the blind quarter straddles p = 2


@pytest.mark.parametrize("sight", [None, SIGHT], ids=["plain", "sight"])
def test_without_the_field_of_view_the_landmark_behind_the_robot_is_pruned(orc, sight):
    """Measured on this drive: pole 0's landmark has evidence 1 4 7 8 6 3 0 at frames 0, 3, .. 18 and is gone from frame 21 on."""
    run = drive(POLES, None, sight)
    got = {f: landmark_of(run[f], POLES[0]) for f in RECORDED}
    print(f"pole 0 without the field of view ({'sight' if sight else 'plain'}): {got}")
    assert got[9] is not None
    for f in RECORDED:
        if f >= 21:
            assert got[f] is None, (f, got)


@pytest.mark.parametrize("sight", [None, SIGHT], ids=["plain", "sight"])
def test_with_the_field_of_view_it_keeps_its_slot(orc, sight):
    run = drive(POLES, FOV, sight)
    got = {f: landmark_of(run[f], POLES[0]) for f in RECORDED}
    outside = [int(fr["outside"].sum()) for fr in run]
    print(f"pole 0 with the field of view ({'sight' if sight else 'plain'}): {got}; outside by frame {outside}")
    for f in RECORDED:
        if f >= 3:
            assert got[f] is not None, (f, got)
    assert got[39] >= got[9]
    assert all(v > 0 for v in outside[30:])
    for f in RECORDED:                                   # and the other poles are where they were
        if f >= 9:
            for k in range(1, len(POLES)):
                assert landmark_of(run[f], POLES[k]) is not None, (f, k)


@pytest.mark.parametrize("sight", [None, SIGHT], ids=["plain", "sight"])
def test_no_pole_leaves_the_arc_nothing_changes(orc, sight):
    off, on = drive(FRONT_POLES, None, sight), drive(FRONT_POLES, FOV, sight)
    assert sum(int(fr["stats"][:, 1].sum()) for fr in off) > 0
    assert all(landmark_of(off[FRAMES - 1], p) is not None for p in FRONT_POLES)
    for f, (a, b) in enumerate(zip(off, on)):
        assert not b["outside"].any(), f
        assert np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32)), f
        assert np.array_equal(a["ev"], b["ev"]) and np.array_equal(a["ev_stats"], b["ev_stats"]), f
        assert np.array_equal(a["anc"], b["anc"]) and np.array_equal(a["logw"].view(np.uint32), b["logw"].view(np.uint32)), f
