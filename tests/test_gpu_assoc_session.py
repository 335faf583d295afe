"""A rows session with data association (slam_pf_assoc_set) against the frame loop restated from the oracle's stage functions
with tests/_assoc_spec.py as its association and landmark stages (_assoc_spec.frame_loop), frame by frame and bit for bit:
poses, map rows, log-weights, ancestors and the view's table and stats — ungated, gated (kept and resampled frames) and
refining; plus the switch's interface: two launches per frame and no fused front, refused off single-GPU rows and under a 2x2
measurement covariance, and switched off again by gate = 0."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
import _shard_worker as W
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES, K = 2048, 160, 4, 24
GATE, NEW_GATE = 9.21, 50.0
GATE_ESS = 0.03   # with this gate the spec resamples frames 0 and 3 and keeps frames 1 and 2
REFINE = (0.05, 0.008727, 1)
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, mp = W.init_state(N, L, lm)
    mp[:, 2, L // 2:] = -1.0                    # the maps start half unseen
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, mp=mp)


def detections(world, f):
    """24 of the world's landmark observations of frame f, in shuffled order and without their ids."""
    _, zx, zy = W.observations(world["lm"], f)
    pick = np.random.default_rng(100 + f).permutation(len(zx))[:K]
    return zx[pick].copy(), zy[pick].copy()


def reference(world, frames=FRAMES, ess=0.0, refine=None):
    return A.frame_loop(world, N, frames, dp=DP, detections=lambda f: detections(world, f), gate=GATE, new_gate=NEW_GATE, create=1,
                        ess=ess, refine=refine, **KW)


def _engine(world):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    return e


def run_session(world, assoc=True, ess=0.0, refine=None, layout="rows", frames=FRAMES, before=None, comm_group=None):
    """One session over `frames` frames.  assoc: slam_pf_assoc_set(GATE, NEW_GATE, 1) in front of frame 0; else the frames read
    the observation table.  before(ses): called on the fresh session first (the refusals).  -> per frame what the reference
    returns, and the counters."""
    pkg = load_package()
    e = _engine(world)
    comm = pkg.Comm.local(e, comm_group, 0) if comm_group else None
    ses = pkg.PfSession(e, N, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    extra = before(pkg, ses) if before else None
    if refine:
        ses.refine_set(*refine)
    if assoc:
        ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(world["x"], world["y"], world["th"])
    ses.set_map(world["mp"])
    fused0, assoc0, forms0, inplace0 = e.frame_fusion_count(), e.assoc_counts(), e.ekf_form_counts(), e.ekf_inplace_form_counts()
    out = []
    for f in range(frames):
        e.obs_upload(*W.observations(world["lm"], f), L)      # (ignored while association is on)
        e.detections_upload(*detections(world, f))
        ses.step(0, DP, True)
        v = ses.device_view()
        e.sync()
        fr = dict(pose=ses.poses(), map=ses.maps(), logw=torch.as_tensor(v["logw"], device=DEV).cpu().numpy(),
                  anc=torch.as_tensor(v["anc"], device=DEV).cpu().numpy() if v["anc"] is not None else None)
        if assoc:
            av = ses.assoc_view()
            fr["assoc"] = torch.as_tensor(av["assoc"], device=DEV).cpu().numpy()
            fr["stats"] = torch.as_tensor(av["stats"], device=DEV).cpu().numpy()
        out.append(fr)
    res = dict(frames=out, fused=e.frame_fusion_count() - fused0, assoc=tuple(np.subtract(e.assoc_counts(), assoc0)),
               forms=tuple(np.subtract(e.ekf_form_counts(), forms0)), inplace=tuple(np.subtract(e.ekf_inplace_form_counts(), inplace0)),
               resampled=ses.frames_resampled(), extra=extra)
    ses.close()
    if comm:
        comm.close()
    e.close()
    return res


def compare(got, want, label, table=True):
    for f, (g, w) in enumerate(zip(got, want)):
        if table:
            assert np.array_equal(g["assoc"][:, :L], w["assoc"]) and np.all(g["assoc"][:, L:] == A.NONE), f"{label} frame {f}: table"
            assert np.array_equal(g["stats"], w["stats"]), f"{label} frame {f}: stats"
        assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label} frame {f}: log-weights"
        ga, wa = (np.arange(len(w["logw"])) if a is None else a for a in (g["anc"], w["anc"]))
        assert np.array_equal(ga, wa), f"{label} frame {f}: ancestors"
        assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label} frame {f}: poses"
        assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label} frame {f}: map rows"


def test_ungated_session_equals_the_spec(world):
    want = reference(world)
    st = np.stack([w["stats"] for w in want])
    assert st[..., 0].sum() > 0 and st[..., 1].sum() > 0 and st[..., 2].sum() > 0   # matches, new landmarks and dropped detections
    got = run_session(world)
    compare(got["frames"], want, "ungated")
    assert got["assoc"] == (FRAMES, FRAMES) and got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0)


def test_gated_session_equals_the_spec(world):
    """The resample gate: the spec alone (checked here, on the CPU) keeps some frames and resamples others; the frame behind a
    kept one associates and updates in place."""
    want = reference(world, ess=GATE_ESS)
    verdicts = [w["resampled"] for w in want]
    assert verdicts == [True, False, False, True], verdicts
    got = run_session(world, ess=GATE_ESS)
    compare(got["frames"], want, "gated")
    assert got["resampled"] == sum(verdicts[:-1])   # the host has looked at every frame but the last
    assert got["assoc"] == (FRAMES, FRAMES) and got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0)


def test_refining_session_equals_the_spec(world):
    want = reference(world, refine=REFINE)
    got = run_session(world, refine=REFINE)
    compare(got["frames"], want, "refining")
    assert got["assoc"] == (FRAMES, FRAMES) and got["fused"] == 0


def _refused(text):
    def before(pkg, ses):
        with pytest.raises(pkg.SlamError) as err:
            ses.assoc_set(GATE, NEW_GATE, True)
        assert err.value.status == -2 and text in str(err.value), str(err.value)
        with pytest.raises(pkg.SlamError) as err:
            ses.assoc_view()
        assert err.value.status == -4
    return before


@pytest.mark.parametrize("layout", ["split", "pages", "auto"])
def test_refused_off_the_row_layout(world, layout):
    """... and the session then steps exactly as one that was never asked."""
    plain = run_session(world, assoc=False, layout=layout, frames=2)
    asked = run_session(world, assoc=False, layout=layout, frames=2, before=_refused("row layout"))
    compare(asked["frames"], plain["frames"], layout, table=False)
    assert asked["assoc"] == (0, 0) and asked["fused"] == plain["fused"]


def test_refused_when_sharded(world):
    pkg = load_package()
    group = pkg.LocalGroup(1)
    plain = run_session(world, assoc=False, frames=2)
    asked = run_session(world, assoc=False, frames=2, before=_refused("not sharded"), comm_group=group)
    group.close()
    compare(asked["frames"], plain["frames"], "sharded", table=False)
    assert asked["assoc"] == (0, 0)


def test_refused_under_a_2x2_covariance_and_the_other_way_round(world):
    cov = (0.02, 0.012, 0.015)

    def before(pkg, ses):
        ses.meas_cov_set(cov)
        _refused("2x2 measurement covariance")(pkg, ses)
        ses.meas_cov_set((KW["meas_var"], 0.0, KW["meas_var"]))
        ses.assoc_set(GATE, NEW_GATE, True)
        with pytest.raises(pkg.SlamError) as err:
            ses.meas_cov_set(cov)
        assert err.value.status == -2 and "data association is on" in str(err.value)
        ses.meas_cov_set((KW["meas_var"], 0.0, KW["meas_var"]))    # the isotropic covariance is no change: accepted
        for bad in ((-1.0, 50.0), (float("nan"), 50.0), (float("inf"), float("inf")), (9.21, 1.0), (9.21, float("nan"))):
            with pytest.raises(pkg.SlamError):
                ses.assoc_set(*bad, True)

    got = run_session(world, frames=2, before=before)                # the refused calls changed nothing: association is on
    compare(got["frames"], reference(world, frames=2), "after the refusals")
    assert got["assoc"] == (2, 2) and got["fused"] == 0


def test_gate_zero_switches_back(world):
    """assoc_set(0) after assoc_set(gate): the session reads the observation table again and runs what a session that never made
    the call runs, bit for bit and through the same kernels."""
    def before(pkg, ses):
        ses.assoc_set(GATE, NEW_GATE, True)
        ses.assoc_set(0.0, 0.0, False)

    plain = run_session(world, assoc=False)
    back = run_session(world, assoc=False, before=before)
    compare(back["frames"], plain["frames"], "switched back", table=False)
    assert back["assoc"] == (0, 0) and back["fused"] == plain["fused"] and back["forms"] == plain["forms"] and back["inplace"] == plain["inplace"]
