"""slam_pf_spread and slam_pose_spread_dev — the mean of a population with its covariance and the length of its mean heading vector —
against their exact restatement (tests/_spread_spec.py, pinned by tests/test_spread_spec_cpu.py), bit for bit in all ten outputs
(the sharded form: tests/test_gpu_spread_session.py).
The session's state (poses, pending ancestors, log-weights) is read through slam_pf_device_view before every call, as
tests/test_gpu_estimates.py does for the mean."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _estimate_spec as E
import _shard_worker as W
import _spread_spec as S
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# one particle, two, a wavefront and its neighbours, more than one workgroup (the mean's launch; the moments' strides from 257 on),
# many workgroups, and the first n at which the 256 workgroups of the mean's launch stride (65 537)
SIZES = [1, 2, 63, 64, 65, 257, 4097, 65537]


def _engine(pkg, world):
    eng = pkg.Engine(0)
    meta, edt, bx, by, _ = world
    d_edt = torch.from_numpy(edt).to(DEV)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    eng.scan_upload(bx, by)
    return eng, d_edt


@pytest.fixture(scope="module")
def rig(orc):
    pkg = load_package()
    world = W.make_world(L=6)
    eng, keep = _engine(pkg, world)
    yield SimpleNamespace(pkg=pkg, eng=eng, world=world, lm=world[4], keep=keep)
    eng.close()


def _session(rig, n, ess=0.0, gain=1.0, eng=None, comm=None):
    return rig.pkg.PfSession(eng or rig.eng, n, 0, seed=E.SEED, sigma=E.SIGMA, meas_var=0.02, score_gain=gain, comm=comm,
                             resample_ess_frac=ess, map_layout="rows")


def _same(got, want):
    """(pose, cov, heading_r) against the restatement's, bit for bit"""
    return all(np.array_equal(bits(np.asarray(g, np.float32)), bits(np.asarray(w, np.float32))) for g, w in zip(got, want[:3]))


def _show(t):
    return [np.asarray(v, np.float32).tolist() for v in t[:3]]


def _dev(*arrays):
    return [None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in arrays]


def _engine_call(rig, x, y, th, ref, idx=None, logw=None):
    """Engine.pose_spread_dev on these arrays -> (what it returned, the restatement's)"""
    n = len(x)
    w16 = carry = None
    if logw is not None:
        w16, _ = E.weights16(logw)
        carry = E.oracle.weight_carry(logw, np.float32(np.fmax.reduce(logw)))
    d = _dev(x, y, th, None if idx is None else np.asarray(idx, np.int32), carry)
    torch.cuda.synchronize()
    got = rig.eng.pose_spread_dev(d[0], d[1], d[2], n, ref, d_idx=d[3], d_carry=d[4])
    return got, S.spread_spec(x, y, th, idx, ref, n, w16)


@pytest.mark.parametrize("n", SIZES)
def test_engine_call_every_size_gathered_and_weighted(rig, n):
    """Plain and weighted, with and without a gather (with repeats, as a resample leaves them), twice each: the accumulators and the
    tickets of both launches come back zeroed."""
    x, y, th = E.edge_population("plain", n)
    rng = np.random.default_rng(n)
    idx = rng.integers(0, n, n)
    logw = rng.normal(-3.0, 1.5, n).astype(np.float32)
    for tag, kw in (("plain", {}), ("gathered", dict(idx=idx)), ("weighted", dict(logw=logw)), ("both", dict(idx=idx, logw=logw))):
        for ref in (0.07, 3.0):
            got, want = _engine_call(rig, x, y, th, ref, **kw)
            assert _same(got, want), (tag, n, ref, _show(got), _show(want))
    if n == 1:
        assert not np.any(bits(want[1])) and want[2] > 0.999999, _show(want)   # +0 six times


POPULATIONS = [(name, "edge") for name in ("plain", "straddle_pi", "negative", "large")] + \
              [(name, "spread") for name in ("two_clusters", "far_cloud", "off_grid", "identical")]


@pytest.mark.parametrize("n", [2049, 65537])
@pytest.mark.parametrize("name,kind", POPULATIONS)
def test_populations_on_their_edges(rig, name, kind, n):
    """The mean's edge populations with their reference headings and the spread's own.  "large" at 2049 particles is 20 km across:
    outside the domain, and the call must say so."""
    x, y, th = E.edge_population(name, n) if kind == "edge" else S.spread_population(name, n)
    for ref in E.REFS.get(name, [0.0, 2.5]):
        try:
            want = S.spread_spec(x, y, th, None, ref, n)
        except S.OutOfDomain:
            assert (name, n) == ("large", 2049)
            with pytest.raises(rig.pkg.SlamError) as err:
                _engine_call(rig, x, y, th, ref)
            assert err.value.status == -2 and "2048 m" in str(err.value)
            continue
        got, _ = _engine_call(rig, x, y, th, ref)
        assert _same(got, want), (name, n, ref, _show(got), _show(want))
        if name == "identical":
            assert not np.any(bits(got[1])) and got[2] > 0.999999, _show(got)
        if name == "two_clusters":
            assert got[2] < 0.01 and abs(got[1][0] - 16.0) < 0.01, _show(got)
        if name == "far_cloud":
            assert 0.5e-4 < got[1][0] < 2e-4, _show(got)


def test_domain_boundary(rig):
    """One particle 2047.9 m from the rest is inside the domain, one 2048.1 m away is outside: SLAM_ERR_INVALID_ARG, and the next
    call is right again (the flag word was cleared with the accumulators)."""
    n = 65537
    # (x ~ 2049 m is beyond the 1024 m of the mean's WEIGHTED form; these calls are plain, and the plain sum of X is far from 2^63 here:
    # 65 536 particles near 1 m and one near 2049 m)
    inside, outside = S.boundary_population(n, 2047.9), S.boundary_population(n, 2048.1)
    got, want = _engine_call(rig, *inside, 0.3)
    assert _same(got, want), (_show(got), _show(want))
    with pytest.raises(S.OutOfDomain):
        S.spread_spec(*outside, None, 0.3, n)
    with pytest.raises(rig.pkg.SlamError) as err:
        _engine_call(rig, *outside, 0.3)
    assert err.value.status == -2 and "1 particles" in str(err.value), str(err.value)
    got, want = _engine_call(rig, *inside, 0.3)
    assert _same(got, want), (_show(got), _show(want))
    ses = _session(rig, n)
    try:
        ses.set_poses(*outside)
        with pytest.raises(rig.pkg.SlamError) as err:
            ses.spread(0.3)
        assert err.value.status == -2
        ses.set_poses(*inside)
        assert _same(ses.spread(0.3), want)
    finally:
        ses.close()


def _state(eng, ses):
    eng.sync()
    v = ses.device_view()
    return [None if v[k] is None else torch.as_tensor(v[k], device=DEV).cpu().numpy() for k in ("pose", "anc", "logw")]


def _check(eng, ses, refs=(0.07,), fq=0, tag=""):
    """mean, spread, spread, mean for every ref against the restatement of the state read just before -> 'k' (the gate kept the last
    frame), 'R' (it resampled) or '|' (no frame yet)"""
    pose, anc, logw = _state(eng, ses)
    n = pose.shape[1]
    kind, w16 = "|" if logw is None else "R", None
    if fq and logw is not None:
        w, wq = E.weights16(logw)
        if not E.gate_resamples(wq, n, fq):
            kind, w16 = "k", w
    for ref in refs:
        want = S.spread_spec(pose[0], pose[1], pose[2], anc, ref, n, w16)
        m0 = ses.mean(ref)
        a = ses.spread(ref)
        b = ses.spread(ref)
        m1 = ses.mean(ref)
        assert _same(a, want) and _same(b, want), (tag, kind, n, ref, _show(a), _show(b), _show(want))
        assert np.array_equal(bits(m0), bits(want[0])) and np.array_equal(bits(m1), bits(want[0])), (tag, kind, n, ref)
    return kind


@pytest.mark.parametrize("n", [1, 65, 4097, 65537])
def test_session_plain_with_and_without_a_pending_gather(rig, n):
    """Before the first step (no gather pending, the plain form), after one step and after three (over pose[anc])."""
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    ses = _session(rig, n)
    try:
        ses.set_poses(x, y, th)
        assert _check(rig.eng, ses, refs=(0.07, -2.0), tag="set_poses") == "|"
        for f in range(3):
            ses.step(0, list(E.DP))
            if f != 1:
                assert _check(rig.eng, ses, refs=(0.07, 3.0), tag=f"frame {f}") == "R"
    finally:
        ses.close()


@pytest.mark.parametrize("n", sorted(E.GATED_SCENARIOS))
def test_gated_session_after_every_step_and_across_the_break(rig, n):
    """The two gated scenarios of the mean: the weighted form on the frames the gate kept, the plain one elsewhere and again after
    the set_poses / reset that follows a kept frame."""
    sc = E.GATED_SCENARIOS[n]
    fq = E.oracle.ess_frac_q16(sc["ess"])
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    ses = _session(rig, n, ess=sc["ess"], gain=sc["gain"])
    kinds = ""
    try:
        ses.set_poses(x, y, th)
        for _ in range(sc["first"]):
            ses.step(0, list(E.DP))
            kinds += _check(rig.eng, ses, refs=(0.0,), fq=fq, tag=f"n={n} after {kinds}")
        assert kinds[-1] == "k"
        if sc["then"] == "reset":
            ses.reset(list(E.RESET_POSE))
        else:
            ses.set_poses(*(a[::-1].copy() for a in ses.poses()))
        kinds += _check(rig.eng, ses, refs=(0.0,), fq=fq, tag="after the break")
        for _ in range(sc["rest"]):
            ses.step(0, list(E.DP))
            kinds += _check(rig.eng, ses, refs=(0.0,), fq=fq, tag=f"n={n} after {kinds}")
    finally:
        ses.close()
    assert "kk" in kinds and "kR" in kinds and "k|" in kinds, kinds
