"""The runs of the assoc-weight tests (test_assoc_weight_spec_cpu.py, test_gpu_assoc_weight_session.py) on the scene of
tests/_pipeline_scenes.py.  TEST INFRASTRUCTURE; numpy and the specifications only, nothing of the package.

The pipeline scene has gate == new_gate (no band between the gates) and 40 slots for eight objects (no particle runs out), so
two runs are added for the two kinds of dropped detection:
  BAND    new_gate = 50: the ghost return, 0.3 m beside its pole, lies beyond gate and within new_gate — dropped with slots free
  SLOTS   L = 6 slots for seven poles and a ghost, gate == new_gate: a detection can only be dropped because no slot is left
"""
import numpy as np

import _assoc_weight_spec as W
import _pipeline_scenes as SC

F = np.float32
CONSTS = (-4.0, -1.5, -0.75)
OTHER = (-0.5, -3.0, -2.0)
BAND_NEW_GATE = 50.0
SLOTS_L = 6

# noise form x evidence form x merging: every form of each at least once; "assoc_weight" a function of the frame where a run changes it
SESSIONS = {
    "iso, no pruning, merge, ess": dict(detections=SC.without_cov, merge_gate=SC.MERGE_GATE, ess=SC.ESS, assoc_weight=CONSTS),
    "2x2, plain pruning, constants change": dict(detections=SC.without_cov, noise=("cov", SC.COV), prune=SC.PRUNE,
                                                 assoc_weight=lambda f: CONSTS if f < 6 else OTHER),
    "detcov, sight, merge, off and on": dict(detections=SC.with_cov, noise=("detcov",), prune=SC.PRUNE, sight=SC.SIGHT, merge_gate=SC.MERGE_GATE,
                                             ess=SC.ESS, assoc_weight=lambda f: None if 4 <= f < 7 else CONSTS),
    "iso, fov, a frame without a hand-over": dict(detections=lambda f: None if f == 5 else SC.without_cov(f), prune=SC.PRUNE, fov=True,
                                                  merge_gate=SC.MERGE_GATE, assoc_weight=CONSTS),
    "whole pipeline": dict(SC.COMBOS["whole pipeline"], assoc_weight=CONSTS),
    "band between the gates": dict(detections=SC.without_cov, prune=SC.PRUNE, sight=SC.SIGHT, fov=True, new_gate=BAND_NEW_GATE, assoc_weight=CONSTS),
}


def run(world, kw, fov_bounds=None, frames=SC.FRAMES):
    """_assoc_weight_spec.frame_loop on the scene with the keywords of a run."""
    kw = dict(kw)
    if kw.get("fov") is True:
        kw["fov"] = tuple(fov_bounds or SC.bounds())
    kw.setdefault("new_gate", SC.NEW_GATE)
    return W.frame_loop(world, SC.SCANS, len(world["x"]), frames, dp=SC.DP, gate=SC.GATE, create=1, **kw, **SC.KW)


def small_world(world, L=SLOTS_L):
    mp = np.zeros((SC.N, 5, L), F)
    mp[:, 2] = -1.0
    return dict(world, mp=mp)


_cache = {}


def reference(world, name, fov_bounds=None):
    key = (name, tuple(float(b) for b in (fov_bounds or SC.bounds())))
    if key not in _cache:
        _cache[key] = run(world, SESSIONS[name], fov_bounds)
    return _cache[key]
