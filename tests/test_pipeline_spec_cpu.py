"""tests/_pipeline_spec.py on the CPU.  (1) With the extra switches off the composed frame loop IS each of the loops it composes:
bit for bit what _fov_spec, _assoc_detcov_spec, _merge_spec and _detect_spec return on their own session tests' configurations —
loops the GPU session already matches.  (2) The combinations of test_gpu_pipeline_session.py are not vacuous: conditions on the
reference alone (tests/_pipeline_scenes.py says how the scene brings them about).  (3) What the loop refuses."""
import numpy as np
import pytest

import _detect_spec as D
import _fov_spec as V
import _pipeline_scenes as SC
import _pipeline_spec as P
import _shard_worker as W
import test_gpu_assoc_detcov_session as TD
import test_gpu_detect_fit_session as TF
import test_gpu_fov_session as TV
import test_gpu_merge_session as TM

F = np.float32


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(u, v) for u, v in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_reduces(got, want, label):
    """Every key of the older loop's frames, bit for bit (det: the points; the composed loop adds the covariances behind them)."""
    assert len(got) == len(want)
    for f, (g, w) in enumerate(zip(got, want)):
        for k, v in w.items():
            assert same(g[k][:len(v)] if k == "det" else g[k], v), f"{label}: frame {f}: {k}"


def empty_world(n, L, orc, scan=False):
    meta, edt, bx, by, _ = W.make_world(L=L)
    x, y, th, _ = W.init_state(n, 0, np.zeros((0, 2), F))
    mp = np.zeros((n, 5, L), F)
    mp[:, 2] = -1.0
    w = dict(meta=meta, edt=edt, x=x, y=y, th=th, mp=mp)
    return dict(w, bx=bx, by=by) if scan else w


@pytest.mark.parametrize("sight", [None, TV.SIGHT], ids=["plain", "sight"])
def test_reduces_to_the_fov_loop(orc, sight):
    meta, edt, _, _, _ = W.make_world(L=TV.L)
    mp = np.zeros((TV.N, 5, TV.L), F)
    mp[:, 2] = -1.0
    world = dict(meta=meta, edt=edt, x=np.zeros(TV.N, F), y=np.zeros(TV.N, F), th=np.zeros(TV.N, F), mp=mp)
    fov = (V.bound(F(TV.ARC[0]) + F(TV.EDGE)), V.bound(F(TV.ARC[1]) - F(TV.EDGE)))
    want = V.frame_loop(world, TV.SCANS, TV.N, dp=TV.DP, gate=TV.GATE, new_gate=TV.NEW_GATE, create=1, prune=TV.PRUNE, fov=fov, sight=sight,
                        detect_params=dict(wrap=0), **TV.KW)
    got = P.frame_loop(world, TV.SCANS, TV.N, TV.FRAMES, dp=TV.DP, gate=TV.GATE, new_gate=TV.NEW_GATE, create=1, prune=TV.PRUNE, fov=fov,
                       sight=sight, detector=dict(params=dict(wrap=0)), **TV.KW)
    assert sum(int(w["outside"].sum()) for w in want) > 0
    assert_reduces(got, want, "fov")


@pytest.mark.parametrize("setup", ["pruning, gated", "refining"])
def test_reduces_to_the_detcov_loop(orc, setup):
    meta, edt, bx, by, lm = W.make_world(L=TD.L)
    x, y, th, mp = W.init_state(TD.N, TD.L, lm)
    mp[:, 2, TD.L // 2:] = -1.0                  # (test_gpu_assoc_session.py: world)
    world = dict(meta=meta, edt=edt, bx=bx, by=by, lm=lm, x=x, y=y, th=th, mp=mp)
    kw = dict(prune=TD.PRUNE, ess=TD.GATE_ESS) if setup.startswith("pruning") else dict(refine=TD.REFINE)
    want = TD.reference(world, **kw)
    got = P.frame_loop(world, None, TD.N, TD.FRAMES, dp=TD.DP, gate=TD.GATE, new_gate=TD.NEW_GATE, create=1, noise=("detcov",),
                       detections=lambda f: TD.feed(world, f), **kw, **TD.KW)
    assert_reduces(got, want, setup)


@pytest.mark.parametrize("setup", list(TM.SETUPS))
def test_reduces_to_the_merge_loop(orc, setup):
    world = empty_world(TM.N, TM.L, orc, scan=True)
    kw = dict(TM.SETUPS[setup])
    want = TM.reference(world, **kw)
    cov = kw.pop("meas_cov", None)
    got = P.frame_loop(world, None, TM.N, TM.FRAMES, dp=TM.DP, gate=TM.GATE, new_gate=TM.NEW_GATE, create=1, detections=TM.detections,
                       merge_gate=TM.MERGE_GATE, noise=("cov", cov) if cov else ("iso",), **kw, **TM.KW)
    assert sum(int(w["merge_stats"][:, 0].sum()) for w in want) > 0
    assert_reduces(got, want, setup)


@pytest.mark.parametrize("prune", [None, TF.PRUNE], ids=["assoc", "pruning"])
def test_reduces_to_the_detect_loop_with_the_fit(orc, prune):
    world = empty_world(TF.N, TF.L, orc)
    want = D.frame_loop(world, TF.SCANS, TF.N, dp=TF.DP, gate=TF.GATE, new_gate=TF.NEW_GATE, create=1, prune=prune, detections=TF.fitted,
                        **TF.KW)
    got = P.frame_loop(world, TF.SCANS, TF.N, TF.FRAMES, dp=TF.DP, gate=TF.GATE, new_gate=TF.NEW_GATE, create=1, prune=prune,
                       detector=dict(fit=TF.FIT), **TF.KW)
    assert_reduces(got, want, "fitted detector")


def test_an_isotropic_2x2_covariance_is_the_isotropic_form(orc):
    """slam_pf_assoc_cov_set with (meas_var, 0, meas_var) is slam_pf_assoc_set: the loop says the same."""
    world = empty_world(TM.N, TM.L, orc, scan=True)
    run = lambda noise: P.frame_loop(world, None, TM.N, 3, dp=TM.DP, gate=TM.GATE, new_gate=TM.NEW_GATE, create=1,
                                     detections=TM.detections, noise=noise, **TM.KW)
    v = TM.KW["meas_var"]
    assert_reduces(run(("cov", (v, 0.0, v))), run(("iso",)), "isotropic Q")


def test_detcov_without_covariances_is_refused(orc):
    """... before anything of the frame runs: uploaded detections without Q_k, and a detector without a noise model."""
    world = SC.make_world()
    kw = dict(dp=SC.DP, gate=SC.GATE, new_gate=SC.NEW_GATE, create=1, noise=("detcov",), **SC.KW)
    with pytest.raises(P.NotReady):
        P.frame_loop(world, SC.SCANS, SC.N, 1, detections=SC.without_cov, **kw)
    with pytest.raises(P.NotReady):
        P.frame_loop(world, SC.SCANS, SC.N, 1, detector=dict(params=SC.PARAMS, fit=SC.FIT), **kw)
    ok = P.frame_loop(world, SC.SCANS, SC.N, 1, detections=lambda f: None, **kw)       # a frame without a hand-over asks for none
    assert ok[0]["assoc"] is None and ok[0]["merge_stats"] is None


# ------------------------------------------------------------------ the combinations of the GPU test are not vacuous
@pytest.fixture(scope="module")
def world(orc):
    return SC.make_world()


@pytest.mark.parametrize("name", list(SC.COMBOS))
def test_combination_is_not_vacuous(world, name):
    SC.check_not_vacuous(world, name)


def test_the_table_is_the_issues(world):
    """Eight rows; every noise form, every detector form, merging behind every evidence stage and behind none, refining and gated
    frames with merging on — and the scene's detections: the ghost beyond the gates, a scan per frame."""
    c = list(SC.COMBOS.values())
    assert len(c) == 8
    assert {k.get("noise", ("iso",))[0] for k in c} == {"iso", "cov", "detcov"}
    assert sum(1 for k in c if k.get("detector")) == 4 and sum(1 for k in c if k.get("merge_gate")) == 7
    assert any(k.get("merge_gate") and k.get("refine") and k.get("ess") and k.get("detector", {}).get("noise") for k in c)
    assert len({SC.SCANS[f][0].tobytes() for f in range(SC.FRAMES)}) == SC.FRAMES
