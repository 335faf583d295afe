"""A rows session with a 2x2 measurement covariance (slam_pf_meas_cov_set) against the frame loop restated from the oracle's stage
functions with tests/_aniso_spec.py as its landmark stage (_aniso_spec.frame_loop), frame by frame and bit for bit: poses, map
rows (slam_pf_get_map_host), log-weights and ancestors — ungated, gated (kept and resampled frames), refining, and three ranks
on one card; plus the setter's interface: no fused front launch, refused off the row layout, and switched off again by
{meas_var, 0, meas_var}."""
import threading

import numpy as np
import pytest
import torch

import _aniso_spec as A
import _shard_worker as W
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 2048, 160, 4
COV = (0.02, 0.012, 0.015)            # correlated
GATE_COV, GATE_ESS = (0.04, 0.0, 4.0), 0.2   # 100 : 1; with this gate the spec keeps frames 1 and 2 and resamples frames 0 and 3
REFINE = (0.05, 0.008727, 1)
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]


@pytest.fixture(scope="module")
def world(orc):
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, mp = W.init_state(N, L, lm)
    return dict(meta=meta, edt=edt, d_edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, mp=mp)


def reference(world, n, covs, ess=0.0, refine=None):
    return A.frame_loop(world, n, len(covs), covs, dp=DP, observations=lambda f: W.observations(world["lm"], f), ess=ess, refine=refine, **KW)


def _engine(world):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["d_edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    return e


def run_session(world, covs, n=N, ess=0.0, refine=None, layout="rows", rank=0, ranks=1, group=None, try_cov=None):
    """One session (or one rank of `ranks`) over len(covs) frames; covs[f] is set in front of frame f wherever it differs from
    frame f - 1's (None: {meas_var, 0, meas_var}).  try_cov: a covariance the session is expected to REFUSE, offered first.
    -> per frame what the reference returns, and the counters."""
    pkg = load_package()
    e = _engine(world)
    comm = pkg.Comm.local(e, group, rank) if group else None
    ses = pkg.PfSession(e, n, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    refused = None
    if try_cov is not None:
        with pytest.raises(pkg.SlamError) as err:
            ses.meas_cov_set(try_cov)
        refused = (err.value.status, str(err.value))
    if refine:
        ses.refine_set(*refine)
    sl = slice(rank * n, (rank + 1) * n)
    ses.set_poses(world["x"][sl], world["y"][sl], world["th"][sl])
    ses.set_map(world["mp"][sl])
    fused0, aniso0, forms0, inplace0 = e.frame_fusion_count(), e.ekf_aniso_count(), e.ekf_form_counts(), e.ekf_inplace_form_counts()
    iso = (KW["meas_var"], 0.0, KW["meas_var"])
    out, last = [], None
    for f, cov in enumerate(covs):
        if cov != last and not (f == 0 and cov is None):
            ses.meas_cov_set(iso if cov is None else cov)
        last = cov
        e.obs_upload(*W.observations(world["lm"], f), L)
        ses.step(0, DP, True)
        v = ses.device_view()
        e.sync()
        logw = torch.as_tensor(v["logw"], device=DEV).cpu().numpy()
        anc = torch.as_tensor(v["anc"], device=DEV).cpu().numpy() if v["anc"] is not None else None
        out.append(dict(pose=ses.poses(), map=ses.maps(), logw=logw, anc=anc))
    res = dict(frames=out, fused=e.frame_fusion_count() - fused0, aniso=e.ekf_aniso_count() - aniso0,
               forms=tuple(np.subtract(e.ekf_form_counts(), forms0)), inplace=tuple(np.subtract(e.ekf_inplace_form_counts(), inplace0)),
               resampled=ses.frames_resampled(), refused=refused)
    ses.close()
    if comm:
        comm.close()
    e.close()
    return res


def compare(got, want, label, ancestors=True):
    for f, (g, w) in enumerate(zip(got, want)):
        assert np.array_equal(bits(g["logw"]), bits(w["logw"])), f"{label} frame {f}: log-weights"
        if ancestors:
            anc = np.arange(len(w["anc"])) if g["anc"] is None else g["anc"]
            assert np.array_equal(anc, w["anc"]), f"{label} frame {f}: ancestors"
        assert np.array_equal(bits(g["pose"]), bits(w["pose"])), f"{label} frame {f}: poses"
        assert np.array_equal(bits(g["map"]), bits(w["map"])), f"{label} frame {f}: map rows"


def test_ungated_session_equals_the_spec(world):
    want = reference(world, N, [COV] * FRAMES)
    got = run_session(world, [COV] * FRAMES)
    compare(got["frames"], want, "ungated")
    assert got["aniso"] == FRAMES and got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0)


def test_gated_session_equals_the_spec(world):
    """The resample gate: the spec alone (checked here, on the CPU) keeps some frames and resamples others; the frame behind a
    kept one updates in place."""
    want = reference(world, N, [GATE_COV] * FRAMES, ess=GATE_ESS)
    verdicts = [w["resampled"] for w in want]
    assert verdicts == [True, False, False, True], verdicts
    got = run_session(world, [GATE_COV] * FRAMES, ess=GATE_ESS)
    compare(got["frames"], want, "gated")
    assert got["resampled"] == sum(verdicts[:-1])   # the host has looked at every frame but the last
    assert got["aniso"] == FRAMES and got["fused"] == 0 and got["forms"] == (0, 0) and got["inplace"] == (0, 0)


def test_refining_session_equals_the_spec(world):
    want = reference(world, N, [COV] * FRAMES, refine=REFINE)
    got = run_session(world, [COV] * FRAMES, refine=REFINE)
    compare(got["frames"], want, "refining")
    assert got["aniso"] == FRAMES and got["fused"] == 0


def test_three_ranks_equal_one_rank_and_the_spec(world):
    """Three ranks of 512 particles on this card (threads of one process, in-process transport): their gather index points into
    the staging tail.  Against one rank of 1 536 and against the spec."""
    pkg = load_package()
    n_total, covs = 1536, [COV] * FRAMES
    want = reference(world, n_total, covs)
    one = run_session(world, covs, n=n_total)
    compare(one["frames"], want, "one rank of 1536")
    group = pkg.LocalGroup(3)
    out, errors = [None] * 3, []

    def rank_main(r):
        try:
            out[r] = run_session(world, covs, n=512, rank=r, ranks=3, group=group)
        except BaseException as exc:   # noqa: BLE001 - re-raised below
            errors.append(exc)

    ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(3)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    group.close()
    if errors:
        raise errors[0]
    joined = [dict(pose=np.concatenate([o["frames"][f]["pose"] for o in out], axis=1), map=np.concatenate([o["frames"][f]["map"] for o in out]),
                   logw=np.concatenate([o["frames"][f]["logw"] for o in out]), anc=None) for f in range(FRAMES)]
    compare(joined, want, "three ranks", ancestors=False)   # (a rank's gather index names local rows and staging rows)
    assert all(o["aniso"] == FRAMES and o["fused"] == 0 for o in out)


def test_switching_back_gives_the_isotropic_update(world):
    """{meas_var, 0, meas_var} after two anisotropic frames: the following frames are orc_ekf_update's, bit for bit, and go
    through the session's usual kernels again."""
    covs = [COV, COV, None, None]
    want = reference(world, N, covs)
    got = run_session(world, covs)
    compare(got["frames"], want, "switched back")
    assert got["aniso"] == 2 and sum(got["forms"]) == 2


@pytest.mark.parametrize("layout,n_landmarks", [("auto", L), ("split", L), ("pages", L), ("split_pages", L), ("rows", 0)])
def test_refused_off_the_row_layout(world, layout, n_landmarks):
    """Only a session created on rows with landmarks keeps a covariance per particle: every other one refuses the call, says why,
    and then steps exactly as a session that was never asked."""
    pkg = load_package()
    if n_landmarks == 0:
        e = _engine(world)
        ses = pkg.PfSession(e, N, 0, map_layout=layout, **KW)
        with pytest.raises(pkg.SlamError) as err:
            ses.meas_cov_set(COV)
        assert err.value.status == -2 and "row layout" in str(err.value)
        ses.set_poses(world["x"], world["y"], world["th"])
        ses.step(0, DP, False)
        want = A.oracle.motion_sample(world["x"], world["y"], world["th"], None, N, 0, DP, KW["sigma"], KW["seed"], 0)
        e.sync()
        v = ses.device_view()
        assert np.array_equal(bits(torch.as_tensor(v["pose"], device=DEV).cpu().numpy()), bits(np.stack(want)))
        ses.close()
        e.close()
        return
    plain = run_session(world, [None, None], layout=layout)
    asked = run_session(world, [None, None], layout=layout, try_cov=COV)
    assert asked["refused"][0] == -2 and "row layout" in asked["refused"][1]
    compare(asked["frames"], plain["frames"], layout, ancestors=False)
    assert asked["aniso"] == 0 and asked["fused"] == plain["fused"]


def test_no_fused_front_while_the_covariance_is_set():
    """A rows session that fuses its front launch (5 000 particles x 300 landmarks) stops doing so once a covariance is set and
    starts again when it is switched off; a covariance that is not positive definite is refused and changes nothing."""
    pkg = load_package()
    n, Lb = 5000, 300
    meta, edt, bx, by, lm = W.make_world(L=Lb)
    x, y, th, mp = W.init_state(n, Lb, lm)
    e = pkg.Engine(0)
    keep = torch.from_numpy(edt).to(DEV)
    e.grid_set_dev(0, keep, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    e.scan_upload(bx, by)
    ses = pkg.PfSession(e, n, Lb, map_layout="rows", **KW)
    ses.set_poses(x, y, th)
    ses.set_map(mp)

    def frames(k0):
        fused, aniso = e.frame_fusion_count(), e.ekf_aniso_count()
        for f in range(k0, k0 + 3):
            z = lm + 0.01 * np.float32(f)
            e.obs_upload(np.arange(Lb, dtype=np.int32), z[:, 0].copy(), z[:, 1].copy(), Lb)
            ses.step(0, DP, True)
        e.sync()
        return e.frame_fusion_count() - fused, e.ekf_aniso_count() - aniso

    assert frames(0) == (2, 0)          # (frame 0 has no pending gather: the front fuses from frame 1 on)
    ses.meas_cov_set(COV)
    assert frames(3) == (0, 3)
    with pytest.raises(pkg.SlamError) as err:
        ses.meas_cov_set((1.0, 1.0, 1.0))
    assert err.value.status == -2 and "meas_cov must be finite" in str(err.value)
    assert frames(6) == (0, 3)
    ses.meas_cov_set((KW["meas_var"], 0.0, KW["meas_var"]))
    assert frames(9) == (3, 0)
    ses.close()
    e.close()
