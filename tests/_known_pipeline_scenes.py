"""The scene and the combinations of the whole known-map tests (test_known_pipeline_spec_cpu.py,
test_gpu_known_pipeline_session.py).  TEST INFRASTRUCTURE; numpy and the specifications only, nothing of the package.

The scene is tests/_pipeline_scenes.py's room of poles under the 269.5-degree, 1079-beam sensor that drives along +y, one ray-cast
scan per frame, 256 particles, 12 frames — with the known maps laid over it:

  MAP_A   12 slots: the seven poles, three empty slots, a PHANTOM where only the passer stands (frames 0, 1: later nothing is
          there and the landmark is missed) and a landmark BEHIND the sensor, in the blind quarter (outside the arc)
  MAP_B   40 slots (the padded stride goes from 32 to 64, the allocation grows): MAP_A's and 28 more, every seventh empty
  BLOCKER the object that stands between the sensor and a pole in frames 4 .. 7: that pole's landmark is spared under line of
          sight, and the blocker itself, like the WALKER of the last frames, is a detection no landmark explains (clutter)
  LONE    frame 9: every pole but one is gone from the scan — the detector finds ONE detection: a pair reseed behind it is a no-op
  BLIND   frame 5 has use_observations == 0: the engine keeps frame 4's detections, and a reseed behind it reads those
"""
import functools

import numpy as np

import _detect_noise_spec as DN
import _detect_spec as D
import _fov_spec as V
import _known_pipeline_spec as KP
import _pipeline_scenes as SC
import _shard_worker as W

F = np.float32
N, FRAMES = 256, 12
KW = dict(seed=5, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.004)
DP = SC.DP
GATE, CLUTTER, LOG_MISS, VIEW_RANGE = 9.21, -2.5, -1.5, 6.0
SIGHT, EDGE, ARC = (128, 0.3), SC.EDGE, SC.ARC
REFINE, ESS = (0.05, 0.008727, 1), 0.5
TOL, MIN_SEP = 0.05, 2.0
PARAMS, FIT, MODEL = SC.PARAMS, SC.FIT, SC.NOISE_MODEL
LONE, BLIND = 9, 5
REF = 0.1
PHANTOM, BEHIND = SC.PASSER, (-3.0, 0.3)


def poles_of(f):
    return SC.POLES[1:2] if f == LONE else SC.poles_of(f)


SCANS = [D.raycast(SC.sensor(f), poles_of(f), SC.RHO, SC.HALF, noise=np.random.default_rng(100 + f), angles=SC.ANGLES)[:2] for f in range(FRAMES)]


def _map(points, empty):
    M = np.zeros((5, len(points)), F)
    M[0], M[1] = np.array(points, F).T
    M[2], M[3], M[4] = 0.05, 0.01, 0.05
    M[2, list(empty)] = -1.0
    return M


_P = [tuple(p) for p in SC.POLES]
_A = [(9.0, 9.0), _P[0], _P[1], _P[2], _P[3], (9.0, -9.0), _P[4], _P[5], _P[6], PHANTOM, (-9.0, 9.0), BEHIND]
MAP_A = _map(_A, (0, 5, 10))
MAP_B = _map(_A + [tuple(p) for p in np.random.default_rng(41).uniform(-5, 5, (28, 2))], (0, 5, 10) + tuple(range(14, 40, 7)))


def bounds():
    """The diamond-angle bounds of ARC as the specification works them out."""
    return V.bound(F(ARC[0]) + F(EDGE)), V.bound(F(ARC[1]) - F(EDGE))


@functools.lru_cache(maxsize=None)
def uploaded(f, cov=False):
    """What a host-side detector hands over in front of frame f: the centroid detector's detections of the frame's scan, shuffled,
    and (cov) the noise model's Q_k of each.  BLIND: nothing."""
    if f == BLIND:
        return None
    zx, zy, k, _ = D.detect(*SCANS[f], **PARAMS)
    pick = np.random.default_rng(900 + f).permutation(k)
    zx, zy = zx[:k][pick].copy(), zy[:k][pick].copy()
    if not cov:
        return zx, zy
    qxx, qxy, qyy, ok = DN.cov_of(zx, zy, MODEL)
    assert ok.all()
    return zx, zy, (qxx, qxy, qyy)


def with_cov(f):
    return uploaded(f, True)


def without_cov(f):
    return uploaded(f, False)


def observing(f):
    return f != BLIND


MISS_RANGE, MISS_ARC, MISS_ALL = (LOG_MISS, VIEW_RANGE, False, None), (LOG_MISS, VIEW_RANGE, True, None), (LOG_MISS, VIEW_RANGE, True, SIGHT)
CENTROID, FITTED, FULL = dict(params=PARAMS), dict(params=PARAMS, fit=FIT), dict(params=PARAMS, fit=FIT, noise=MODEL)
MODELLED = dict(params=PARAMS, noise=MODEL)
single = lambda fr: ("single", fr)
pairs = lambda fr: ("pairs", fr, TOL, MIN_SEP)
SINGLE = {1: single(0.25), 3: single(1.0 / 16), BLIND: single(0.5), 7: single(1.0), LONE: single(0.5), 10: single(2.0**-10)}
PAIRS = {1: pairs(0.25), 3: pairs(1.0 / 16), BLIND: pairs(0.5), 7: pairs(1.0), LONE: pairs(1.0), 10: pairs(0.5)}
BOTH = {1: [single(0.25), pairs(0.5)], 3: pairs(0.25), BLIND: single(0.25), 7: [pairs(1.0), single(0.25)], LONE: [pairs(1.0), single(0.5)],
        10: [pairs(0.5), pairs(0.5)]}
# behind every change of a switch (frames 2, 3, 4, 6, 7, 8), the lone frame, and a no-op in front of a step
SWITCHED = {2: single(0.25), 3: pairs(0.5), 4: single(0.5), 6: pairs(1.0), 7: single(0.25), 8: pairs(0.25), LONE: [pairs(1.0), single(0.5)]}

# every key a keyword of _known_pipeline_spec.frame_loop
COMBOS = {
    "iso uploaded single": dict(detections=without_cov, reseed_after=SINGLE.get),
    "iso fitted pairs": dict(detector=FITTED, reseed_after=PAIRS.get),
    "detcov modelled miss+arc+sight single": dict(noise=("detcov",), detector=MODELLED, miss=MISS_ALL, reseed_after=SINGLE.get),
    "detcov uploaded+Qk refine pairs ess": dict(noise=("detcov",), detections=with_cov, refine=REFINE, ess=ESS, reseed_after=PAIRS.get),
    "iso uploaded miss refine both ess": dict(detections=without_cov, miss=MISS_ARC, refine=REFINE, ess=ESS, reseed_after=BOTH.get),
    "everything": dict(noise=("detcov",), detector=FULL, miss=MISS_ALL, refine=REFINE, ess=ESS, reseed_after=BOTH.get),
    "everything, switching": dict(noise=lambda f: ("iso",) if 3 <= f < 6 else ("detcov",), regive=(6,), detector=FULL,
                                  known_map=lambda f: MAP_B if 4 <= f < 8 else MAP_A,
                                  miss=lambda f: None if f < 2 else MISS_RANGE if f < 4 else MISS_ARC if f < 7 else MISS_ALL,
                                  tries=lambda f: ["model"] if f == 4 else [], refine=REFINE, ess=ESS, reseed_after=SWITCHED.get),
    "everything, restart": dict(noise=("detcov",), detector=FULL, miss=MISS_ALL, refine=REFINE, ess=ESS, reseed_after=BOTH.get, restart=(6,),
                                tries=lambda f: ["reseed-off", "miss-off"] if f == 6 else []),
}


def make_world():
    """(the oracle must have been built: the `orc` fixture)"""
    meta, edt, _, _, _ = W.make_world(L=1)
    return dict(meta=meta, edt=edt, x=np.zeros(N, F), y=np.zeros(N, F), th=np.zeros(N, F))


def schedule(name):
    """The keywords of a combination, completed with what all of them share."""
    kw = dict(known_map=MAP_A, observing=observing, ref=REF)
    kw.update(COMBOS[name])
    return kw


def run(world, kw, arc=None, frames=FRAMES):
    return KP.frame_loop(world, SCANS, N, frames, dp=DP, gate=GATE, log_clutter=CLUTTER, arc=tuple(arc or bounds()), **kw, **KW)


_cache = {}


def reference(world, name, arc=None):
    """The reference of a combination, computed once per process and left unchanged."""
    key = (name, tuple(float(b) for b in (arc or bounds())))
    if key not in _cache:
        _cache[key] = run(world, schedule(name), arc)
    return _cache[key]


def facts(want):
    """What a reference run holds, for the conditions that keep a combination from being vacuous."""
    tot = lambda k, col=None: sum(int((w[k] if col is None else w[k][:, col]).sum()) for w in want if w[k] is not None)
    calls = [(w["resampled"], r) for w in want for r in w["reseeds"][:1]]
    cnt = lambda kind, i: sum(r["counts"][i] for w in want for r in w["reseeds"] if r["call"][0] == kind)
    return dict(matched=tot("stats", 0), clutter=tot("stats", 2), missed=tot("missed"), spared=tot("spared"), outside=tot("outside"),
                ndet=[len(w["det"][0]) if w["det"] is not None else 0 for w in want], observing=[w["stats"] is not None for w in want],
                single=[cnt("single", i) for i in range(2)], pairs=[cnt("pairs", i) for i in range(4)],
                noops=[f for f, w in enumerate(want) for r in w["reseeds"] if r["reseeded"] is None],
                resampled=[bool(w["resampled"]) for w in want],
                reseed_behind_kept=sum(1 for res, r in calls if not res and r["reseeded"] is not None),
                reseed_behind_resampled=sum(1 for res, r in calls if res and r["reseeded"] is not None),
                refused=[(f, w["refused"]) for f, w in enumerate(want) if w["refused"]])


def check_not_vacuous(world, name, arc=None):
    """The conditions on the reference of one combination (asserted again at the top of the GPU test): every branch the
    combination has switched on is taken somewhere in its run."""
    kw = schedule(name)
    fa = facts(reference(world, name, arc))
    print(name, fa)
    at = lambda k, f: kw[k](f) if callable(kw.get(k)) else kw.get(k)
    assert fa["matched"] > 0, "no matched pair"
    assert fa["clutter"] > 0, "no unmatched detection"
    assert fa["observing"].count(False) == 1 and not fa["observing"][BLIND], "one non-observing frame"
    miss = [at("miss", f) for f in range(FRAMES)]
    if any(miss):
        assert fa["missed"] > 0, "no landmark is missed"
        if any(m and m[2] for m in miss):
            assert fa["outside"] > 0, "no landmark lies outside the arc"
        if any(m and m[3] for m in miss):
            assert fa["spared"] > 0, "line of sight spares no landmark"
    if kw.get("detector"):
        few = [f for f, k in enumerate(fa["ndet"]) if k < 2]
        assert few == [LONE] and at("reseed_after", LONE) is not None, "fewer than two detections on exactly the lone frame, which is reseeded"
        assert sum(k >= 2 for k in fa["ndet"]) >= FRAMES - 2
    kinds = {c[0] for f in range(FRAMES) for c in ([at("reseed_after", f)] if not isinstance(at("reseed_after", f), list) else at("reseed_after", f)) if c}
    if "single" in kinds:
        assert all(v > 0 for v in fa["single"]), ("a single-reseed count stays 0", fa["single"])
    if "pairs" in kinds:
        assert all(v > 0 for v in fa["pairs"]), ("a pair-reseed count stays 0", fa["pairs"])
        assert LONE in fa["noops"], "no pair reseed is a no-op"
    if kw.get("ess"):
        assert any(fa["resampled"]) and not all(fa["resampled"]), fa["resampled"]
        assert fa["reseed_behind_kept"] > 0 and fa["reseed_behind_resampled"] > 0, "a reseed behind a kept AND behind a resampled frame"
    return fa
