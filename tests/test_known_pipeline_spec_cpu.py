"""tests/_known_pipeline_spec.py on the CPU.  (1) With the extra switches off the composed loop IS each of the five loops it
composes — _localise_spec, _localise_detcov_spec, _localise_miss_spec, _reseed_spec, _reseed_pair_spec — bit for bit and frame by
frame on their own session tests' scenes and arguments: loops the GPU session already matches.  (2) The combinations of
test_gpu_known_pipeline_session.py are not vacuous: conditions on the reference alone (tests/_known_pipeline_scenes.py says how
the scene brings them about).  (3) A refused frame or call leaves the loop's state untouched."""
import numpy as np
import pytest

import _known_pipeline_scenes as KS
import _known_pipeline_spec as KP
import _localise_detcov_spec as LD
import _localise_miss_spec as MS
import _localise_spec as LS
import _reseed_pair_spec as RP
import _reseed_spec as R
import _shard_worker as W
import test_gpu_localise_miss_session as TM
import test_gpu_localise_session as TL
import test_gpu_reseed_pairs_session as TP
import test_gpu_reseed_session as TR
from test_pipeline_spec_cpu import same

F = np.float32


def known_world(n, L, every):
    """The world of the known-map session tests: W.make_world's room and landmarks, every `every`-th slot of the map empty."""
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, _ = W.init_state(n, 0, np.zeros((0, 2), F))
    M = np.zeros((5, L), F)
    M[0], M[1], M[2], M[4] = lm[:, 0], lm[:, 1], 0.05, 0.05
    M[3] = 0.01
    M[2, ::every] = -1.0
    return dict(meta=meta, edt=edt, bx=bx, by=by, lm=lm, x=x, y=y, th=th, M=M)


def assert_reduces(got, want, label, keys=None):
    """Every key of the older loop's frames, bit for bit."""
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            if keys is None or k in keys:
                assert same(g[k], v), f"{label}: frame {f}: {k}"


def composed(world, n, frames, kw, scans=None, **schedule):
    kw = dict(kw)
    kw.setdefault("meas_var", 1.0)   # (not read under the per-detection form)
    return KP.frame_loop(world, scans or [(world["bx"], world["by"])] * frames, n, frames, **kw, **schedule)


@pytest.mark.parametrize("refine", [None, TL.REFINE], ids=["plain", "refined"])
@pytest.mark.parametrize("ess", [0.0, TL.GATE_ESS], ids=["every-frame", "gated"])
def test_reduces_to_the_localise_loop(orc, ess, refine):
    """... with the mode switched off from frame 4 on and a frame without observations, as its session test has them."""
    world = known_world(TL.N, TL.L, 7)
    known = lambda f: world["M"] if f < 4 else None
    det = lambda f: TL.detections(world, f) if f != 2 else None
    want = LS.frame_loop(world, TL.N, TL.FRAMES, dp=TL.DP, detections=det, known_map=known, gate=TL.GATE, log_clutter=TL.CLUTTER, ess=ess,
                         refine=refine, **TL.KW)
    got = composed(world, TL.N, TL.FRAMES, dict(TL.KW, dp=TL.DP, gate=TL.GATE, log_clutter=TL.CLUTTER, ess=ess, refine=refine),
                   detections=det, known_map=known)
    assert sum(w["stats"] is not None for w in want) == 3
    assert_reduces(got, want, "localise")


@pytest.mark.parametrize("ess", [0.0, TL.GATE_ESS], ids=["every-frame", "gated"])
def test_reduces_to_the_detcov_loop(orc, ess):
    world = known_world(TL.N, TL.L, 7)
    det = lambda f: TM.detections(world, f, True)
    kw = {k: v for k, v in TL.KW.items() if k != "meas_var"}
    want = LD.frame_loop(world, TL.N, TL.FRAMES, dp=TL.DP, detections=det, known_map=world["M"], gate=TL.GATE, log_clutter=TL.CLUTTER, ess=ess, **kw)
    got = composed(world, TL.N, TL.FRAMES, dict(kw, dp=TL.DP, gate=TL.GATE, log_clutter=TL.CLUTTER, ess=ess), detections=det,
                   known_map=world["M"], noise=("detcov",))
    assert_reduces(got, want, "detcov")


@pytest.mark.parametrize("detcov", [False, True], ids=["iso", "detcov"])
def test_reduces_to_the_miss_loop(orc, detcov):
    """... with the detector's scans (line of sight reads every frame's own), refining, the misses stepped through their views."""
    world = known_world(TM.N, TM.L, 7)
    scans, kws, M = TL.scans_and_map()
    arc = KS.bounds()
    views = [None, (TM.LOG_MISS, TM.VIEW_RANGE, False, None), (TM.LOG_MISS, TM.VIEW_RANGE, True, None), (TM.LOG_MISS, TM.VIEW_RANGE, True, TM.SIGHT)]
    mine = lambda f: views[min(f, 3)]
    theirs = lambda f: None if mine(f) is None else (mine(f)[0], mine(f)[1], arc if mine(f)[2] else None, mine(f)[3])
    det = lambda f: TM.detections(world, f, detcov)
    kw = {k: v for k, v in TL.KW.items() if k != "meas_var"}
    want = MS.frame_loop(world, TM.N, TM.FRAMES, dp=TL.DP, detections=det, known_map=M, gate=TL.GATE, log_clutter=TL.CLUTTER,
                         meas_var=None if detcov else TL.KW["meas_var"], miss=theirs, refine=TL.REFINE, scans=scans, **kw)
    got = composed(world, TM.N, TM.FRAMES, dict(kw, meas_var=TL.KW["meas_var"], dp=TL.DP, gate=TL.GATE, log_clutter=TL.CLUTTER, refine=TL.REFINE,
                                                arc=arc), scans=scans, detections=det, known_map=M, miss=mine,
                   noise=("detcov",) if detcov else ("iso",))
    assert sum(int(w["spared"].sum()) for w in want[3:]) >= 0 and sum(int(w["missed"].sum()) for w in want[1:]) > 0
    assert_reduces(got, want, "miss")


@pytest.mark.parametrize("detcov", [False, True], ids=["meas-var", "per-detection"])
@pytest.mark.parametrize("ess", [0.0, TR.GATE_ESS], ids=["every-frame", "gated"])
def test_reduces_to_the_reseed_loops(orc, ess, detcov):
    """Both reseed loops on their session tests' scene: counts and reseeded populations as well."""
    n = TP.N
    world = known_world(n, TR.L, 5)
    det = lambda f: TR.detections(world, f, detcov)
    kw = dict(TR.spec_kw(detcov), dp=TR.DP, gate=TR.GATE, log_clutter=TR.CLUTTER, ess=ess)
    form = ("detcov",) if detcov else ("iso",)
    want = R.frame_loop(world, n, TR.FRAMES, detections=det, known_map=world["M"], reseed_after=TR.FRACTIONS.get, **kw)
    got = composed(world, n, TR.FRAMES, kw, detections=det, known_map=world["M"], noise=form,
                   reseed_after=lambda f: ("single", TR.FRACTIONS[f]) if f in TR.FRACTIONS else None)
    assert sum(w["counts"] is not None for w in want) == len(TR.FRACTIONS)
    assert_reduces(got, want, "reseed")
    want = RP.frame_loop(world, n, TP.FRAMES, detections=det, known_map=world["M"], reseed_after=TP.FRACTIONS.get, tol=TP.TOL, min_sep=TP.MIN_SEP, **kw)
    got = composed(world, n, TP.FRAMES, kw, detections=det, known_map=world["M"], noise=form,
                   reseed_after=lambda f: ("pairs", TP.FRACTIONS[f], TP.TOL, TP.MIN_SEP) if f in TP.FRACTIONS else None)
    assert_reduces(got, want, "reseed from pairs")


@pytest.fixture(scope="module")
def world(orc):
    return KS.make_world()


@pytest.mark.parametrize("name", list(KS.COMBOS))
def test_combinations_are_not_vacuous(world, name):
    KS.check_not_vacuous(world, name)


def test_the_scene_takes_every_branch_somewhere(world):
    """Over the combinations the GPU test runs: both noise forms, every miss view, every detector form, both maps, a refused
    frame, a refused model, a refused reseed — and the facts the issue lists, each named."""
    fa = {name: KS.facts(KS.reference(world, name)) for name in KS.COMBOS}
    every = fa["everything"]
    assert every["matched"] > 0 and every["clutter"] > 0
    assert every["missed"] > 0 and every["spared"] > 0 and every["outside"] > 0
    assert [f for f, k in enumerate(every["ndet"]) if k < 2] == [KS.LONE] and sum(k >= 2 for k in every["ndet"]) >= KS.FRAMES - 2
    assert every["observing"].count(False) == 1
    assert all(v > 0 for v in every["single"]) and all(v > 0 for v in every["pairs"])
    assert every["reseed_behind_kept"] > 0 and every["reseed_behind_resampled"] > 0
    assert fa["everything, switching"]["refused"] == [(4, ["model"]), (6, ["frame"])]
    assert fa["everything, restart"]["refused"] == [(6, ["reseed-off", "miss-off"])]
    sw = KS.reference(world, "everything, switching")
    assert sw[3]["det"][2] is None and sw[2]["det"][2] is not None and sw[6]["det"][2] is not None   # the model dropped, and given again
    assert sw[4]["assoc"].shape[1] == 40 and sw[8]["assoc"].shape[1] == 12                            # the larger map and back


def test_a_refused_frame_leaves_the_loop_as_it_was(world):
    """The refused frame of the switching run (the detector lost its model under the isotropic form) against a run whose host
    gave the model again in front of the frame and never saw a refusal; and without either, the loop refuses for good."""
    kw = KS.schedule("everything, switching")
    asked = KS.reference(world, "everything, switching")
    never = KS.run(world, dict(kw, regive=(), redetect=(6,), tries=None))
    for f, (a, b) in enumerate(zip(asked, never)):
        for k in ("pose", "logw", "anc", "stats", "missed", "spared", "outside", "det", "reads", "reseeds"):
            assert same_deep(a[k], b[k]), (f, k)
    assert asked[-1]["session"].frames_resampled == never[-1]["session"].frames_resampled
    with pytest.raises(KP.NotReady, match="frame 6"):
        KS.run(world, dict(kw, regive=(), tries=None), frames=7)


def test_refused_calls_leave_the_loop_as_it_was(world):
    """The restart run's refused reseed and misses (the mode is off) against a run that never tried them."""
    kw = KS.schedule("everything, restart")
    asked = KS.reference(world, "everything, restart")
    never = KS.run(world, dict(kw, tries=None))
    for f, (a, b) in enumerate(zip(asked, never)):
        for k in ("pose", "logw", "anc", "stats", "det", "reads", "reseeds"):
            assert same_deep(a[k], b[k]), (f, k)
    # ... and the restart shows: a run that never switched the map off carries on with the same state, as the rules say — the
    # switches given again are the switches that were there
    straight = KS.run(world, dict(kw, tries=None, restart=()))
    assert all(same_deep(a[k], b[k]) for a, b in zip(asked, straight) for k in ("pose", "logw", "anc"))
    ses = KP.Session(world, KS.N, **KS.KW)
    for call in (lambda: ses.miss_set(KS.MISS_RANGE), lambda: ses.detect_set(KS.FITTED)):
        with pytest.raises(KP.InvalidArg):
            call()
    with pytest.raises(KP.NotReady):
        ses.reseed(("single", 0.5))
    ses.known_map_set(KS.MAP_A, "iso", KS.GATE, KS.CLUTTER)
    with pytest.raises(KP.NotReady, match="no detections"):
        ses.reseed(("single", 0.5))
    with pytest.raises(KP.InvalidArg, match="noise model"):
        ses.detect_set(KS.FULL)
    ses.known_map_set(KS.MAP_A, "detcov", KS.GATE, KS.CLUTTER)
    ses.detect_set(KS.FULL)
    ses.known_map_set(KS.MAP_B, "iso", KS.GATE, KS.CLUTTER)
    assert ses.detector == KS.FITTED | dict(noise=None)          # the model is dropped, the detector stays
    ses.known_map_set(None)
    assert ses.detector is None and ses.miss is None              # the map off takes both along


def same_deep(a, b):
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_deep(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return isinstance(b, (tuple, list)) and len(a) == len(b) and all(same_deep(u, v) for u, v in zip(a, b))
    if a is None or b is None or isinstance(a, (str, bool, int, float)):
        return a is b or a == b
    return same(a, b)
