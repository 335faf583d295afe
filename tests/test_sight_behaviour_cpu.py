"""Line-of-sight evidence (tests/_sight_spec.py) as a rule: a drive past a pole that hides another.  The chain detector ->
association -> update -> evidence on the spec loops, in a box room with six poles; for nineteen frames pole 1 at (2, .6) stands
between the sensor and pole 0 at (4, .6).  With the evidence of tests/_evidence_spec.py the hidden pole's landmark takes a miss in
every such frame, is pruned, and is learnt again; with the sight table it keeps its slot, its mean and its evidence.  And a room in
which nothing hides anything gives the same maps and evidence either way.  No GPU."""
import numpy as np
import pytest

import _detect_spec as D
import _sight_spec as S

RHO, HALF, NBEAMS = 0.1, 6.0, 360
POLES = np.array([(4, .6), (2, .6), (3, -2), (-3, 1), (1, 3.5), (-2, -3)], np.float64)
OPEN_POLES = np.array([(4, .6), (0.5, -3), (-3, -2), (-3, 2.5), (1, 3.5)], np.float64)   # no pole passes behind another
N, SLOTS, FRAMES = 64, 8, 40
DP = (0.0, 0.03, 0.0)
KW = dict(seed=5, sigma=(0.005, 0.005, 0.001), meas_var=2.5e-3, score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
PRUNE = (1, 1, 8, 9.0)
SIGHT = (128, 0.3)
RECORDED = tuple(range(0, FRAMES, 5)) + (FRAMES - 1,)


def scans_of(poles):
    return [D.raycast((0.0, 0.03 * (f + 1), 0.0), poles, RHO, HALF, NBEAMS, noise=np.random.default_rng(100 + f))[:2] for f in range(FRAMES)]


def drive(poles, sight):
    world = dict(x=np.zeros(N, np.float32), y=np.zeros(N, np.float32), th=np.zeros(N, np.float32), mp=np.zeros((N, 5, SLOTS), np.float32))
    world["mp"][:, 2] = -1.0
    return S.frame_loop(world, scans_of(poles), N, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, prune=PRUNE, sight=sight, score=False, **KW)


def heaviest(fr):
    """-> (map row, evidence row) of the frame's heaviest particle (it survives the resample)."""
    k = int(np.flatnonzero(fr["anc"] == np.argmax(fr["logw"]))[0])
    return fr["map"][k], fr["ev"][k]


def landmark_of(fr, pole):
    """The evidence of the landmark of the heaviest particle within 0.3 m of the pole's centre, None: there is none."""
    row, ev = heaviest(fr)
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen] - pole[0], row[1, seen] - pole[1])
    near = seen[d <= 0.3]
    return int(ev[near[0]]) if len(near) else None


@pytest.fixture(scope="module")
def runs(orc):
    return drive(POLES, None), drive(POLES, SIGHT)


def test_the_drive_hides_pole_0(runs):
    """What the test is about: for a stretch of frames the detector gives nothing at pole 0, before and after it does."""
    def detected(f):
        zx, zy = (v.astype(np.float64) for v in runs[0][f]["det"])
        return bool(np.any(np.hypot(zx - POLES[0, 0], zy + 0.03 * (f + 1) - POLES[0, 1]) <= 0.3))
    assert detected(5) and detected(35)
    assert not any(detected(f) for f in range(10, 29))


def test_a_hidden_landmark_keeps_its_slot(runs):
    """Measured on this drive: without sight pole 0's landmark is gone from the heaviest particle at frames 20 and 25 and back at 30
    with evidence 2; with sight (128, 0.3) it is there in every recorded frame from 10 on with evidence 8."""
    plain, sight = runs
    cmax = PRUNE[2]
    got = {f: (landmark_of(plain[f], POLES[0]), landmark_of(sight[f], POLES[0])) for f in RECORDED}
    prunes = [sum(int(fr["ev_stats"][:, 0].sum()) for fr in run) for run in runs]
    spared = sum(int(fr["spared"].sum()) for fr in sight)
    print(f"pole 0 (evidence without, with sight) by frame: {got}; prunes {prunes[0]} -> {prunes[1]}; spared {spared}")
    assert got[20][0] is None
    for f in RECORDED:
        if f >= 10:
            assert got[f][1] is not None, f
    assert got[20][1] == cmax and got[25][1] == cmax
    for f in RECORDED:
        if f >= 10:
            for k in range(1, len(POLES)):
                assert landmark_of(plain[f], POLES[k]) is not None and landmark_of(sight[f], POLES[k]) is not None, (f, k)
    assert prunes[1] <= prunes[0]
    assert spared > 0


def test_nothing_hidden_nothing_changes(orc):
    """A room in which no pole passes behind another: the two rules give the same maps and the same evidence, frame for frame."""
    plain, sight = drive(OPEN_POLES, None), drive(OPEN_POLES, SIGHT)
    assert sum(int(fr["stats"][:, 1].sum()) for fr in plain) > 0
    for f, (a, b) in enumerate(zip(plain, sight)):
        assert np.array_equal(a["map"].view(np.uint32), b["map"].view(np.uint32)), f
        assert np.array_equal(a["ev"], b["ev"]) and np.array_equal(a["ev_stats"], b["ev_stats"]), f
        assert np.array_equal(a["anc"], b["anc"]), f
