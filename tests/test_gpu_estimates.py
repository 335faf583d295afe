"""slam_pf_mean and slam_pf_best — what a host takes out of a session — against their exact restatement (tests/_estimate_spec.py,
pinned by tests/test_estimate_spec_cpu.py), bit for bit.  Everything goes through PfSession; the poses, the pending ancestors and
the log-weights are read through slam_pf_device_view before every call, and the restatement is computed from those."""
import threading
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _estimate_spec as E
import _shard_worker as W
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# a wavefront, a workgroup, the one-workgroup arg-max and its 1024-stride loop, the first n at which the 256 workgroups of the
# pose sums stride (65 537), and one well beyond
SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2049, 65536, 65537, 200000]


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


def _session(rig, n, L=0, ess=0.0, gain=1.0, layout="rows", eng=None, comm=None):
    return rig.pkg.PfSession(eng or rig.eng, n, L, seed=E.SEED, sigma=E.SIGMA, meas_var=0.02, score_gain=gain, comm=comm,
                             resample_ess_frac=ess, map_layout=layout)


def _state(eng, ses):
    """pose [3][n], the pending ancestors (None: no gather pending) and the log-weights (None: no frame yet) as the device holds them"""
    eng.sync()
    v = ses.device_view()
    return [None if v[k] is None else torch.as_tensor(v[k], device=DEV).cpu().numpy() for k in ("pose", "anc", "logw")]


def _same(a, b):
    return np.array_equal(bits(a), bits(b))


def _check(eng, ses, refs=(0.07,), fq=0, tag=""):
    """mean (for every ref) and best against the restatement of the state read just before -> 'k' (the gate kept the last frame),
    'R' (it resampled) or '|' (no frame yet)"""
    pose, anc, logw = _state(eng, ses)
    n = pose.shape[1]
    kind, w16 = "|" if logw is None else "R", None
    if fq and logw is not None:
        w, wq = E.weights16(logw)
        if not E.gate_resamples(wq, n, fq):
            kind, w16 = "k", w
    for ref in refs:
        want, _ = E.mean_spec(pose[0], pose[1], pose[2], anc, ref, n, w16)
        got = ses.mean(ref)
        assert _same(got, want), (tag, kind, n, ref, got.tolist(), want.tolist())
    if logw is not None:   # (before the first frame the view shows no log-weights: there is no heaviest particle to restate)
        _check_best(ses, logw, pose, tag)
    return kind


def _check_best(ses, logw, pose, tag="", first_id=0):
    wp, wv, wi = E.best_spec(logw, pose[0], pose[1], pose[2], first_id)
    gp, gv, gi = ses.best()
    assert gi == wi and _same(gv, wv) and _same(gp, wp), (tag, gi, wi, float(gv), float(wv), gp.tolist(), wp.tolist())


@pytest.mark.parametrize("n", SIZES)
def test_every_size_in_three_states(rig, n):
    """After set_poses (no gather pending: idx == nullptr), after one step (over pose[anc]) and after three."""
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


@pytest.mark.parametrize("ess,gain", [(0.0, 1.0), (0.5, 0.1)])
def test_repeated_and_interleaved_calls(rig, ess, gain):
    """The accumulators and the ticket are cleared by every call, best and mean share one result block and one sequence number,
    and the next frame is the same whether anybody asked or not.  Gated: frames 2 and 3 are kept, so the nine weighted sums are in play
    between calls that use four."""
    n, frames = 2049, 5
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    fq = E.oracle.ess_frac_q16(ess)
    quiet = _session(rig, n, ess=ess, gain=gain)
    try:
        quiet.set_poses(x, y, th)
        silent = []
        for f in range(frames):
            quiet.step(0, list(E.DP))
            silent.append(quiet.poses())       # (a getter of the product, but not one of the two calls under test)
    finally:
        quiet.close()
    ses = _session(rig, n, ess=ess, gain=gain)
    kinds = ""
    try:
        ses.set_poses(x, y, th)
        _check(rig.eng, ses, refs=(0.07, 0.07, -1.0, 0.07))
        for f in range(frames):
            ses.step(0, list(E.DP))
            assert _same(ses.poses(), silent[f]), f
            kinds += _check(rig.eng, ses, refs=(0.07, 0.07, -1.0, 2.5, 0.07), fq=fq, tag=f"frame {f} mean x5, best")
            pose, anc, logw = _state(rig.eng, ses)
            _check_best(ses, logw, pose)                       # best, best, mean, best, mean, mean, best
            _check_best(ses, logw, pose)
            _check(rig.eng, ses, refs=(0.3,), fq=fq)
            _check(rig.eng, ses, refs=(0.3, -0.3), fq=fq)
    finally:
        ses.close()
    assert ("k" in kinds and "R" in kinds) if ess else kinds == "R" * frames, kinds


@pytest.mark.parametrize("n", [2049, 65537])
@pytest.mark.parametrize("name", ["plain", "straddle_pi", "negative", "large"])
def test_pose_populations_on_their_edges(rig, name, n):
    """The populations tests/test_estimate_spec_cpu.py proves to sit on their edges, with ref_theta up to +-pi off and through the
    range reduction of det_sincos; then one frame, so that the same goes through the gather ("large" stays where it is: its
    poses are a million metres off the grid, nothing a frame is specified for)."""
    x, y, th = E.edge_population(name, n)
    ses = _session(rig, n)
    try:
        ses.set_poses(x, y, th)
        _check(rig.eng, ses, refs=E.REFS[name], tag=name)
        if name != "large":
            ses.step(0, list(E.DP))
            _check(rig.eng, ses, refs=E.REFS[name], tag=name + " + frame")
    finally:
        ses.close()


@pytest.mark.parametrize("n", [2049, 65537])
def test_best_ties_infinities_and_nan(rig, n):
    """Log-weights written through the view (no entry point produces these on demand): tied maxima inside a wavefront, across
    wavefronts and across the 1024-stride loop, a -inf tail, one NaN — in front of, and in place of, the maximum — and nothing
    but -inf and NaN."""
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    ses = _session(rig, n)
    try:
        ses.set_poses(x, y, th)
        ses.step(0, list(E.DP))
        pose, anc, logw = _state(rig.eng, ses)
        d_logw = torch.as_tensor(ses.device_view()["logw"], device=DEV)
        rng = np.random.default_rng(n)
        inf, nan = np.float32(np.inf), np.float32(np.nan)
        base = rng.normal(-5.0, 1.0, n).astype(np.float32)
        cases = {}
        for tag, where in (("one wavefront", [70, 75]), ("two wavefronts", [1500, 700, 701]), ("the 1024-stride", [2048, 1024 + 33, 1024]), ("one thread of it", [2048, 1024]),
                           ("both ends", [n - 1, 0]), ("late", [n - 1, n - 2])):
            lw = base.copy()
            lw[where] = 1.5
            cases["tie in " + tag] = lw
        lw = base.copy(); lw[n // 3:] = -inf; cases["-inf tail"] = lw
        lw = base.copy(); lw[:n - 5] = -inf; cases["-inf head"] = lw
        lw = base.copy(); lw[[900, 40]] = 2.0; lw[3] = nan; cases["NaN before the maximum"] = lw
        lw = base.copy(); lw[int(np.argmax(base))] = nan; cases["NaN where the maximum was"] = lw
        cases["all -inf"] = np.full(n, -inf, np.float32)
        lw = np.full(n, -inf, np.float32); lw[0] = nan; lw[5::7] = nan; cases["NaN first, else -inf and NaN"] = lw
        cases["all NaN"] = np.full(n, nan, np.float32)
        for tag, lw in cases.items():
            d_logw.copy_(torch.from_numpy(lw))
            torch.cuda.synchronize()
            _check_best(ses, lw, pose, tag)
    finally:
        ses.close()


@pytest.mark.parametrize("layout", ["rows", "split", "pages", "split_pages"])
def test_every_layout(rig, layout):
    """The estimates do not depend on how the maps are kept: one shape, L = 6, three frames with observations."""
    n, L = 2049, 6
    x, y, th, mp = W.init_state(n, L, rig.lm)
    ses = _session(rig, n, L=L, gain=0.05, layout=layout)
    try:
        ses.set_poses(x, y, th)
        ses.set_map(mp)
        _check(rig.eng, ses)
        for f in range(3):
            rig.eng.obs_upload(*W.observations(rig.lm, f), L)
            ses.step(0, list(E.DP), True)
            assert ses.layout() == layout
            _check(rig.eng, ses, refs=(0.07, 3.0), tag=f"{layout} frame {f}")
    finally:
        ses.close()


@pytest.mark.parametrize("n", sorted(E.GATED_SCENARIOS))
def test_gated_session_weighs_the_frames_it_keeps(rig, n):
    """resample_ess_frac in (0, 1), frame by frame: the verdict from orc_ess_resample on the view's log-weights, the ancestors the
    identity exactly on kept frames, the mean the WEIGHTED restatement there and the plain one elsewhere — and plain again after
    the set_poses / reset that follows a kept frame (stale weights).  test_estimate_spec_cpu.py proves that the scenario has
    kept frames in a row, a resample behind a kept frame, the break behind a kept frame, and a kept frame whose two means are
    more than 16 ulps apart."""
    sc = E.GATED_SCENARIOS[n]
    fq = E.oracle.ess_frac_q16(sc["ess"])
    x, y, th, _ = W.init_state(n, 0, rig.lm[:0])
    ses = _session(rig, n, ess=sc["ess"], gain=sc["gain"])
    kinds, ident = "", np.arange(n, dtype=np.int32)

    def frame():
        ses.step(0, list(E.DP))
        kind = _check(rig.eng, ses, refs=(0.0, 0.07), fq=fq, tag=f"n={n} after {kinds}")
        anc = _state(rig.eng, ses)[1]
        assert np.array_equal(anc, ident) == (kind == "k"), (kinds, kind)
        return kind

    try:
        ses.set_poses(x, y, th)
        for _ in range(sc["first"]):
            kinds += frame()
        assert kinds[-1] == "k"
        if sc["then"] == "reset":
            ses.reset(list(E.RESET_POSE))
        else:
            ses.set_poses(*(a[::-1].copy() for a in ses.poses()))
        kinds += _check(rig.eng, ses, refs=(0.0, 0.07), fq=fq, tag="after the break")   # no log-weights in the view: plain
        for _ in range(sc["rest"]):
            kinds += frame()
    finally:
        ses.close()
    assert "kk" in kinds and "kR" in kinds and "k|" in kinds, kinds


def _ranks(rig, world, n_total, ess, gain, frames, refs):
    """`world` ranks on this card (one host thread and one engine per rank, in-process transport; world == 1: a plain session)
    -> per rank, per frame: [mean for every ref..., best]; for one rank also the restatement's."""
    pkg = rig.pkg
    n = n_total // world
    x, y, th, _ = W.init_state(n_total, 0, rig.lm[:0])
    group = pkg.LocalGroup(world) if world > 1 else None
    out, errors = [None] * world, []

    def rank_main(r):
        comm = None
        try:
            eng, keep = (rig.eng, None) if world == 1 else _engine(pkg, rig.world)
            comm = pkg.Comm.local(eng, group, r) if group else None
            ses = _session(rig, n, ess=ess, gain=gain, eng=eng, comm=comm)
            sl = slice(r * n, (r + 1) * n)
            ses.set_poses(x[sl], y[sl], th[sl])
            rec = []
            for f in range(frames):
                ses.step(0, list(E.DP))
                if world == 1:   # the restatement, from the state of the whole population
                    kind = _check(eng, ses, refs=refs, fq=E.oracle.ess_frac_q16(ess), tag=f"one rank, frame {f}")
                    rec.append([kind])
                else:
                    rec.append([])
                rec[-1] += [ses.mean(ref) for ref in refs] + [ses.best()]
            out[r] = rec
            ses.close()
            if comm:
                comm.close()
            if world > 1:
                eng.close()
        except BaseException as exc:   # noqa: BLE001 - re-raised by the caller
            errors.append(exc)
            if comm:
                comm.abort()             # the other ranks fail instead of waiting

    if world == 1:
        rank_main(0)
    else:
        ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
        group.close()
    if errors:
        raise errors[0]
    return out


@pytest.mark.parametrize("ess,gain", [(0.0, 1.0), (0.5, 0.1)])
def test_three_ranks_equal_one_rank_equal_the_restatement(rig, ess, gain):
    """n_total = 12 288 as 3 ranks sharing this card against one rank, the mean and the heaviest particle after every frame: every
    rank returns the same bits, the index is the global id, and the one rank's are the restatement's (checked inside)."""
    n_total, frames, refs = 12288, 8, (0.07, -2.0)
    one = _ranks(rig, 1, n_total, ess, gain, frames, refs)[0]
    many = _ranks(rig, 3, n_total, ess, gain, frames, refs)
    kinds = "".join(rec[0] for rec in one)
    assert ("k" in kinds and "R" in kinds) if ess else kinds == "R" * frames, kinds
    ids = set()
    for f in range(frames):
        want = one[f][1:]
        for r in range(3):
            got = many[r][f]
            for k in range(len(refs)):
                assert _same(got[k], want[k]), (f, r, k, kinds)
            assert got[-1][2] == want[-1][2] and _same(got[-1][1], want[-1][1]) and _same(got[-1][0], want[-1][0]), (f, r)
        ids.add(want[-1][2] * 3 // n_total)
    print("gate:", kinds, "heaviest particle on ranks", sorted(ids))
