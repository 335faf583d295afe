"""Does existence evidence (tests/_evidence_spec.py: frame_loop) keep a map clean that association alone lets clutter fill?  The
drive of test_assoc_behaviour_cpu.py (12 true landmarks, 16 slots, 40 frames, 256 particles, no grid) with C false detections
per frame, uniform in +-8 m, behind the shuffled true ones.  No GPU.  The assertions are conditions, not tolerances."""
import numpy as np
import pytest

import _evidence_spec as E
from test_assoc_behaviour_cpu import DP, GATE, KW, NEW_GATE, drive, yardstick

N, L_TRUE, SLOTS, FRAMES = 256, 12, 16, 40
PRUNE = (1, 1, 8, 9.0)    # hit, miss, cmax, view_range
CONFIRMED = 3             # a landmark of the heaviest particle counts once its evidence is >= 3


@pytest.fixture(scope="module")
def scene():
    return drive()


@pytest.fixture(scope="module")
def ref_rms(orc, scene):
    """RMS distance to the truth of the known-correspondence filter's heaviest particle."""
    lm, frames = scene
    row = yardstick(orc, frames)
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen, None] - lm[None, :, 0], row[1, seen, None] - lm[None, :, 1])
    assert len(seen) == L_TRUE
    return float(np.sqrt(np.mean(np.min(d, axis=1) ** 2)))


def run(scene, C, cseed, prune):
    """-> (row [5][SLOTS] and evidence [SLOTS] (None without pruning) of the heaviest particle of the last frame, prunes over the
    whole population and drive)."""
    _, frames = scene
    rng = np.random.default_rng(cseed)   # one generator for the whole drive

    def detections(f):
        _, zx, zy, perm = frames[f]
        clutter = rng.uniform(-8, 8, (C, 2)).astype(np.float32)
        return np.concatenate([zx[perm], clutter[:, 0]]), np.concatenate([zy[perm], clutter[:, 1]])

    world = dict(x=np.zeros(N, np.float32), y=np.zeros(N, np.float32), th=np.zeros(N, np.float32), mp=np.zeros((N, 5, SLOTS), np.float32))
    world["mp"][:, 2] = -1.0
    out = E.frame_loop(world, N, FRAMES, dp=DP, detections=detections, gate=GATE, new_gate=NEW_GATE, create=1, score=False,
                       prune=prune, **KW)
    last = out[-1]
    k = int(np.flatnonzero(last["anc"] == np.argmax(last["logw"]))[0])   # (the heaviest particle survives the resample)
    pruned = sum(int(o["ev_stats"][:, 0].sum()) for o in out) if prune else 0
    return last["map"][k], last["ev"][k] if prune else None, pruned


def nearest(row, slots, lm):
    d = np.hypot(row[0, slots, None] - lm[None, :, 0], row[1, slots, None] - lm[None, :, 1])
    return np.argmin(d, axis=1), np.min(d, axis=1)


@pytest.mark.parametrize("cseed", [7, 8])
@pytest.mark.parametrize("C", [1, 2])
def test_clutter_fills_the_map_without_pruning_and_not_with_it(scene, ref_rms, C, cseed):
    """Measured (C in {1, 2}, cseed in {7, 8}): without pruning all 16 slots in use, the farthest 2.66-2.96 m from anything real;
    with pruning 12 confirmed landmarks, RMS 0.0096-0.0259 m against the yardstick's 0.0241 m, 6 400-8 455 prunes."""
    lm, _ = scene
    row, _, _ = run(scene, C, cseed, None)
    seen = np.flatnonzero(~(row[2] < 0))
    _, dist = nearest(row, seen, lm)
    print(f"C={C} cseed={cseed} without pruning: {len(seen)} seen, farthest {dist.max():.2f} m")
    assert len(seen) == SLOTS and dist.max() > 1.0, (len(seen), dist.max())

    row, ev, pruned = run(scene, C, cseed, PRUNE)
    conf = np.flatnonzero(~(row[2] < 0) & (ev >= CONFIRMED))
    who, dist = nearest(row, conf, lm)
    rms = float(np.sqrt(np.mean(dist ** 2)))
    print(f"C={C} cseed={cseed} with pruning: {len(conf)} confirmed, rms {rms:.4f} m (yardstick {ref_rms:.4f} m), {pruned} prunes")
    assert len(conf) == L_TRUE and len(np.unique(who)) == L_TRUE, (len(conf), who)
    assert rms <= 2.0 * ref_rms, (rms, ref_rms)   # the bound of test_assoc_behaviour_cpu.py: beyond it lies a wrong association
    assert pruned > 0


def test_clean_input_loses_nothing(scene):
    """C = 0: early misses of true landmarks (evidence 1 after the first sighting, missed in the next frame) cost 256 prunes
    over the population and nothing else."""
    row, ev, pruned = run(scene, 0, 7, PRUNE)
    seen = ~(row[2] < 0)
    print(f"C=0: {int(seen.sum())} seen, {int((seen & (ev >= CONFIRMED)).sum())} confirmed, {pruned} prunes")
    assert seen.sum() == L_TRUE and (seen & (ev >= CONFIRMED)).sum() == L_TRUE
    assert pruned == 256


def test_the_range_gates_the_rule(scene):
    """view_range = 4.0 on the C = 2 drive: nothing is pruned and the map stays full."""
    row, _, pruned = run(scene, 2, 7, (1, 1, 8, 4.0))
    assert pruned == 0 and (~(row[2] < 0)).sum() == SLOTS
