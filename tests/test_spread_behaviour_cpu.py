"""What slam_pf_spread tells a host during global localisation, with the specification's frame loop (tests/_localise_spec.py) and
the restatement of the spread (tests/_spread_spec.py) on the scene of tests/test_localise_behaviour_cpu.py, seeds 1 .. 5: the
position spread sqrt(cov_xx + cov_yy) of the cloud the first frame starts from — spread over the whole map — against that of the
last frame's population.  The bound and every figure: profiles/spread.md.  Needs no GPU."""
import numpy as np
import pytest

import _localise_detcov_spec as SD
import _localise_spec as L
import _spread_spec as S
import test_localise_detcov_behaviour_cpu as BD
from test_localise_behaviour_cpu import CLUTTER, FRAMES, GATE, KW, N, scene

SEEDS = (1, 2, 3, 4, 5)
# metres: twice the worst of seeds 1 .. 5 (0.1606 m, seed 5; profiles/spread.md).  The floor is the motion noise a frame adds behind
# its resample: sigma = 0.08 m per axis, sqrt(2) * 0.08 = 0.113 m
BOUND = 0.3212


def position_spread(x, y, th):
    _, cov, r, _ = S.spread_spec(x, y, th, None, 0.0, len(x))
    return float(np.sqrt(float(cov[0]) + float(cov[2]))), float(r)


@pytest.fixture(scope="module")
def runs(orc):
    out = {}
    for seed in SEEDS:
        M, _, dp, detections, cloud = scene(seed)
        frames = L.frame_loop(cloud, N, FRAMES, seed=seed, dp=dp, detections=detections, known_map=M, gate=GATE, log_clutter=CLUTTER,
                              score=False, **KW)
        out[seed] = (position_spread(cloud["x"], cloud["y"], cloud["th"]), position_spread(*frames[0]["pose"]),
                     position_spread(*frames[-1]["pose"]))
    return out


def test_the_spread_narrows_as_the_cloud_settles(runs):
    """The last frame against the cloud the first frame starts from, and against the population behind the first frame's resample —
    except for seed 3, where that resample keeps a single particle: a population of clones has a spread of exactly 0 until the next
    frame's motion noise, so the figure is printed and not asserted there."""
    for seed, (start, first, last) in runs.items():
        print(f"seed {seed}: position spread {start[0]:.4f} m (heading_r {start[1]:.4f}) at the start, {first[0]:.4f} m behind the first "
              f"frame's resample, {last[0]:.4f} m (heading_r {last[1]:.6f}) at the last frame")
        assert last[0] < start[0], seed
        if seed != 3:                                           # (seed 3: clones, 0 m; see above)
            assert last[0] < first[0], seed
        assert last[0] < BOUND, seed
        assert start[1] < 0.1 and last[1] > 0.99, seed          # headings: all round the circle, then one


def test_a_small_spread_is_agreement_not_correctness(orc):
    """Recorded for the reader, not asserted against the bound: seed 5 of tests/test_localise_detcov_behaviour_cpu.py's scene settles
    7.5 m from the truth, and its spread says "settled" like any other."""
    M, truth, dp, detections, cloud = BD.scene(5)
    frames = SD.frame_loop(cloud, N, FRAMES, detections=detections, seed=5, dp=dp, known_map=M, gate=GATE, log_clutter=CLUTTER, score=False,
                           **BD.KW)
    last = position_spread(*frames[-1]["pose"])
    est = frames[-1]["pose"][:2].astype(np.float64).mean(axis=1)
    err = float(np.hypot(*(est - truth[FRAMES, :2])))
    print(f"per-detection scene, seed 5: position spread {last[0]:.4f} m, heading_r {last[1]:.6f}, error of the mean {err:.3f} m")
    assert err > 10 * last[0]
