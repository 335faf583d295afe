"""The scene and the combinations of the whole-pipeline tests (test_pipeline_spec_cpu.py, test_gpu_pipeline_session.py).  TEST
INFRASTRUCTURE; numpy and the specifications only, nothing of the package.

The scene is the field-of-view session's: the 269.5-degree, 1079-beam sensor (wrap = 0) drives along +y through a square room
with poles, one ray-cast scan per frame.  It is arranged so that twelve frames hold everything the stages react to:

  LEAVING    a pole beside the blind quarter: the drive takes it out of the arc after a few frames (field of view: outside)
  PASSER     a pole-sized object that stands in the room during the first frames only (its landmark is pruned later) ...
  BLOCKER    ... and another that steps between the sensor and a pole for some frames (line of sight: that pole is spared)
  WALKER     ... and a third that walks through the last frames, WALKER_STEP a frame: further than the association's gates
             reach, so every frame starts a new landmark on it and leaves the last one behind — a duplicate in every particle,
             which the merge fuses into the new landmark and which, without merging, lingers until its evidence is used up.
             (A duplicate that only SOME particles start — the detector's noise against a tight gate — costs them the
             likelihood term of a match: they lose the next resample, and the final maps would not tell the two runs apart.)
  GHOST      uploaded detections carry, in every frame, a second return of one pole displaced by GHOST_OFFSET, beyond the
             association's gates (tests/test_gpu_merge_session.py); the detector cannot be handed one
"""
import functools

import numpy as np

import _detect_noise_spec as DN
import _detect_spec as D
import _fov_spec as V
import _pipeline_spec as P
import _shard_worker as W

F = np.float32
N, L, FRAMES = 300, 40, 12
KW = dict(seed=5, sigma=(0.02, 0.02, 0.004), meas_var=2.5e-3, score_gain=0.004)
DP = [0.0, 0.03, 0.0]
GATE, NEW_GATE, MERGE_GATE = 9.21, 9.21, 40.0
PRUNE = (2, 1, 4, 9.0)
SIGHT = (128, 0.3)
EDGE = 0.1
COV = (4e-3, 1e-3, 2.5e-3)
REFINE = (0.05, 0.008727, 2)
ESS = 0.5
RHO, HALF = 0.1, 6.0
FIT = (RHO, 0.0)
NOISE_MODEL = (2.5e-3, 1.5625e-4, 2.5e-3)
PARAMS = dict(wrap=0)
ANGLES = -2.351831 + 0.004363 * np.arange(1079)
ARC = (float(F(ANGLES[0])), float(F(ANGLES[-1])), EDGE)
POLES = np.array([(-0.911, 1.213), (3, -2), (4, .6), (1, 3.5), (2.5, 3), (-1, -2.5), (1.5, -3.5)], np.float64)
PASSER, PASSER_FRAMES = (2.0, -0.8), range(0, 2)
BLOCKER, BLOCKER_FRAMES = (2.0, 0.4), range(4, 8)
WALKER, WALKER_STEP, WALKER_FRAMES = (2.0, 1.6), 0.25, range(8, FRAMES)
GHOST_OFFSET = 0.3


def poles_of(f):
    extra = [PASSER] * (f in PASSER_FRAMES) + [BLOCKER] * (f in BLOCKER_FRAMES)
    if f in WALKER_FRAMES:
        extra.append((WALKER[0] + WALKER_STEP * (f - WALKER_FRAMES[0]), WALKER[1]))
    return np.concatenate([POLES, np.array(extra, np.float64).reshape(-1, 2)])


def sensor(f):
    return (0.0, DP[1] * (f + 1), 0.0)


SCANS = [D.raycast(sensor(f), poles_of(f), RHO, HALF, noise=np.random.default_rng(100 + f), angles=ANGLES)[:2] for f in range(FRAMES)]


def bounds():
    """The diamond-angle bounds of ARC as the specification works them out."""
    return V.bound(F(ARC[0]) + F(EDGE)), V.bound(F(ARC[1]) - F(EDGE))


@functools.lru_cache(maxsize=None)
def uploaded(f, ghost=True, cov=False):
    """What a host-side detector would hand over for frame f: the centroid detector's detections of the frame's scan, shuffled,
    with (ghost) a displaced second return of one of them, and (cov) the noise model's Q_k of each."""
    rng = np.random.default_rng(900 + f)
    zx, zy, k, _ = D.detect(*SCANS[f], **PARAMS)
    z = np.stack([zx[:k], zy[:k]], 1)
    if ghost:
        a = rng.uniform(0, 2 * np.pi)
        g = z[f % k] + F(GHOST_OFFSET) * np.array([np.cos(a), np.sin(a)], F)
        z = np.concatenate([z, g[None]])
    z = z[rng.permutation(len(z))].astype(F)
    zx, zy = z[:, 0].copy(), z[:, 1].copy()
    if not cov:
        return zx, zy
    qxx, qxy, qyy, ok = DN.cov_of(zx, zy, NOISE_MODEL)
    assert ok.all()
    return zx, zy, (qxx, qxy, qyy)


def with_cov(f):
    return uploaded(f, True, True)


def without_cov(f):
    return uploaded(f, True, False)


# the minimum table of the issue, row by row; every key a keyword of _pipeline_spec.frame_loop ("fov": True = the arc's bounds)
COMBOS = {
    "uploaded+Qk detcov sight+fov": dict(detections=with_cov, noise=("detcov",), prune=PRUNE, sight=SIGHT, fov=True, merge_gate=MERGE_GATE),
    "uploaded 2x2 sight ess": dict(detections=without_cov, noise=("cov", COV), prune=PRUNE, sight=SIGHT, merge_gate=MERGE_GATE, ess=ESS),
    "uploaded iso fov refine": dict(detections=without_cov, prune=PRUNE, fov=True, merge_gate=MERGE_GATE, refine=REFINE),
    "centroid iso sight+fov ess": dict(detector=dict(params=PARAMS), prune=PRUNE, sight=SIGHT, fov=True, merge_gate=MERGE_GATE, ess=ESS),
    "fitted 2x2 fov": dict(detector=dict(params=PARAMS, fit=FIT), noise=("cov", COV), prune=PRUNE, fov=True, merge_gate=MERGE_GATE),
    "whole pipeline": dict(detector=dict(params=PARAMS, fit=FIT, noise=NOISE_MODEL), noise=("detcov",), prune=PRUNE, sight=SIGHT, fov=True,
                           merge_gate=MERGE_GATE, refine=REFINE, ess=ESS),
    "whole pipeline, no merge": dict(detector=dict(params=PARAMS, fit=FIT, noise=NOISE_MODEL), noise=("detcov",), prune=PRUNE, sight=SIGHT,
                                     fov=True),
    "uploaded+Qk detcov no evidence": dict(detections=with_cov, noise=("detcov",), merge_gate=MERGE_GATE, refine=REFINE, ess=ESS),
}


def make_world():
    """(the oracle must have been built: the `orc` fixture)"""
    meta, edt, _, _, _ = W.make_world(L=L)
    mp = np.zeros((N, 5, L), F)
    mp[:, 2] = -1.0                              # the maps start empty
    return dict(meta=meta, edt=edt, x=np.zeros(N, F), y=np.zeros(N, F), th=np.zeros(N, F), mp=mp)


def run(world, kw, fov_bounds=None, frames=FRAMES):
    """_pipeline_spec.frame_loop on the scene with the keywords of a combination."""
    kw = dict(kw)
    if kw.get("fov") is True:
        kw["fov"] = tuple(fov_bounds or bounds())
    return P.frame_loop(world, SCANS, N, frames, dp=DP, gate=GATE, new_gate=NEW_GATE, create=1, **kw, **KW)


_cache = {}


def reference(world, name, fov_bounds=None, merge=True):
    """The reference of a combination, computed once per process (merge = False: the same run with merge_gate = 0)."""
    key = (name, tuple(float(b) for b in (fov_bounds or bounds())), merge)
    if key not in _cache:
        kw = dict(COMBOS[name])
        if not merge:
            kw["merge_gate"] = 0.0
        _cache[key] = run(world, kw, fov_bounds)
    return _cache[key]


def facts(want):
    """What a reference run holds, for the conditions that keep a combination from being vacuous."""
    tot = lambda k, col=None: sum(int((w[k] if col is None else w[k][:, col]).sum()) for w in want if w[k] is not None)
    # a merge that moved a non-zero evidence byte: a byte that was not 0 behind the evidence stage and is 0 behind the merge (the
    # stage writes two bytes per merge: the anchor's, which only grows, and the absorbed slot's, which becomes 0)
    moved = sum(int(((w["ev_stage"] > 0) & (w["ev_raw"] == 0)).sum()) for w in want if w["merge_stats"] is not None and w["ev_stage"] is not None)
    return dict(moved=moved, pruned=[int(w["ev_stats"][:, 0].sum()) if w["ev_stats"] is not None else 0 for w in want], spared=tot("spared"),
                outside=tot("outside"), merged=tot("merge_stats", 0), refused=tot("merge_stats", 1),
                resampled=[bool(w["resampled"]) for w in want], seen=int((~(want[-1]["map"][:, 2] < 0)).sum()),
                created=tot("stats", 1), matched=tot("stats", 0))


def check_not_vacuous(world, name, fov_bounds=None):
    """The conditions on the reference of one combination (asserted again at the top of the GPU test)."""
    kw = COMBOS[name]
    fa = facts(reference(world, name, fov_bounds))
    print(name, fa)
    assert fa["created"] > 0 and fa["matched"] > 0
    if kw.get("prune"):
        assert max(fa["pruned"]) > 0, "no frame prunes a landmark"
        if kw.get("sight"):
            assert fa["spared"] > 0, "line of sight spares no landmark"
        if kw.get("fov"):
            assert fa["outside"] > 0, "no landmark lies outside the arc"
    if kw.get("merge_gate"):
        off = facts(reference(world, name, fov_bounds, merge=False))
        assert fa["merged"] > 0 and fa["seen"] < off["seen"], (fa["merged"], fa["seen"], off["seen"])
        if kw.get("prune"):
            assert fa["moved"] > 0, "no merge moves a non-zero evidence byte"
    if kw.get("ess"):
        assert any(fa["resampled"]) and not all(fa["resampled"]), fa["resampled"]
