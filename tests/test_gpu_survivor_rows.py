"""Survivor rows (slam_survivor_rows_set; csrc/ekf_split_body.h MEANS / TALLY, ekf_materialise_kernel, pf_session_store.hip: settle_means):
on the split layout the fused front launch of a single-GPU session that resamples every frame writes no mean row, a launch
behind the resample writes the rows of the particles it kept, and anything else that looks at mean rows first has them all
written.  No result may depend on the switch.

The comparison partner is the same session with the switch OFF — today's frame, which tests/test_gpu_frame_front_at_size.py
pins to the CPU specification (orc_ekf_update) — compared as bit patterns, and the CPU specification itself for the rows
read through the pending gather with no settle in between.

Shapes: the smallest at which the fused front still runs and every tail is partial — n = 4099 (a last group of 3 particles),
L = 261 (plane stride 288: a partial second pass of 256 landmarks) —, bench.py's world as in _front_frames of
test_gpu_frame_front_at_size.py, maps with several dozen covariance classes and landmarks nobody has seen yet (P_xx = -1 on
a stride), some landmarks unobserved in some frames.  PARITY UNPINNED: the reference has no landmarks.
"""
import functools

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GRID, BEAMS, SEED = 1024, 360, 1234
N, L = 4099, 261
LP = (L + 31) // 32 * 32
NFRAMES = 16


def _tensor(a):
    return torch.as_tensor(a, device=DEV)


@functools.lru_cache(maxsize=None)
def _world():
    """bench.py's room, landmarks and frames, the EDT, the initial population — made once, never changed."""
    import bench as B

    pkg = load_package()
    rng = np.random.default_rng(4321)
    landmarks = B.make_landmarks(L, rng)
    pixel, min_x, min_y = np.float32(20.48 / GRID), np.float32(-4.24), np.float32(-10.24)
    occ = B.occupancy(GRID, float(pixel), float(min_x), float(min_y))
    fr = B.make_frames(NFRAMES, BEAMS, landmarks, rng, 0)
    for f in (2, 4):                                   # some landmarks unobserved (NaN in the table), whole batches among them
        keep = ~np.isin(fr[f]["ids"], np.concatenate([np.arange(7, L, 5), np.arange(128, 256)] if f == 4 else [np.arange(7, L, 5)]))
        fr[f] = dict(fr[f], ids=fr[f]["ids"][keep], zx=fr[f]["zx"][keep], zy=fr[f]["zy"][keep])
    sparse = B.make_frames(NFRAMES, BEAMS, landmarks, np.random.default_rng(99), 32)   # the 32 nearest observed
    eng = pkg.Engine(0)
    d_edt = torch.empty((GRID, GRID), dtype=torch.float32, device=DEV)
    eng.edt_dev(torch.from_numpy(occ).to(DEV), GRID, GRID, GRID, 10.0, d_edt)
    eng.sync()
    eng.close()
    g = torch.Generator(device="cpu").manual_seed(SEED)
    p0 = B.true_pose(0)
    poses = [(p0[k] + s * torch.randn(N, generator=g)).numpy().astype(np.float32) for k, s in ((0, 0.05), (1, 0.05), (2, 0.01))]
    m0 = torch.zeros((N, 5, LP), dtype=torch.float32, device=DEV)
    torch.manual_seed(7)
    B.fill_maps(torch, m0, landmarks, L, DEV, N)
    fam = torch.zeros(N, dtype=torch.long)             # runs of 1 .. 96 neighbouring particles share their covariances: the classes
    i, frng = 0, np.random.default_rng(3)
    while i < N:
        k = int(frng.integers(1, 97))
        fam[i:i + k] = i
        i += k
    a = 0.2 * torch.randn((N, 4, L), device=DEV)
    m0[:, 2, :L] = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + 0.02
    m0[:, 3, :L] = a[:, 0] * a[:, 2] + a[:, 1] * a[:, 3]
    m0[:, 4, :L] = a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3] + 0.02
    m0[:, 2, 5:L:17] = -1.0                            # first sightings
    m0[:, 2:5] = m0[fam.to(DEV), 2:5]
    torch.cuda.synchronize()
    assert len(torch.unique(fam)) >= 36
    return dict(B=B, fr=fr, sparse=sparse, d_edt=d_edt, meta=(pixel, min_x, min_y), poses=poses, m0=m0, m0_host=m0.cpu().numpy())


def _session(on, layout="split", ess=0.0):
    w = _world()
    B, pkg = w["B"], load_package()
    eng = pkg.Engine(0)
    eng.survivor_rows_set(on)
    eng.profile_enable(eng.PROF_MATERIALISE)           # (the front launch stays fused: only SLAM_PROF_SCORE splits it)
    eng.grid_set_dev(0, w["d_edt"], pkg.grid_meta(GRID, GRID, GRID, *w["meta"]))
    ses = pkg.PfSession(eng, N, L, sigma=B.SIGMA, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN, seed=SEED, map_layout=layout,
                        resample_ess_frac=ess)
    ses.set_poses(*w["poses"])
    ses.set_map_dev(w["m0"], 5 * LP, LP)
    eng.sync()
    return eng, ses


def _step(eng, ses, fr, use_obs=True):
    eng.scan_upload(fr["bx"], fr["by"])
    eng.obs_upload(fr["ids"], fr["zx"], fr["zy"], L)
    ses.step(0, fr["dp"], use_obs)


def _view_state(eng, ses):
    """what a frame left, read from the session's own buffers (asks for the views: settles)"""
    eng.sync()
    v = ses.device_view()
    out = {k: _tensor(v[k]).cpu().numpy() for k in ("pose", "score", "logw", "anc") if v[k] is not None}
    if v["loglik"] is not None:
        out["loglik"] = _tensor(v["loglik"]).cpu().numpy()
    if ses.layout() == "split":
        sv = ses.split_view()
        out["mean"] = _tensor(sv["mean"])[:N].cpu().numpy()
        out["cls"] = _tensor(sv["cls"])[:N].cpu().numpy()
        used = np.unique(out["cls"])
        out["cov"] = _tensor(sv["cov"])[torch.from_numpy(used).to(DEV).long()].cpu().numpy()
        out["covx"] = _tensor(sv["covx"])[torch.from_numpy(used).to(DEV).long()].cpu().numpy()   # their determinant terms
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k}"


def _final(eng, ses):
    out = {"maps": ses.maps(), "poses": ses.poses(), "best": np.concatenate([np.ravel(p) for p in ses.best()])}
    return out


def _close(*pairs):
    for eng, ses in pairs:
        ses.close()
        eng.close()


def test_on_equals_off_frame_by_frame():
    w = _world()
    on, off = _session(True), _session(False)
    for f in range(6):
        for eng, ses in (on, off):
            _step(eng, ses, w["fr"][f])
        _assert_same(_view_state(*on), _view_state(*off), f"frame {f}")
    # every frame but the first (no gather index yet) was a survivor frame: its own launch + one settle for the views
    assert on[0].profile_read(on[0].PROF_MATERIALISE)[1] == 2 * 5
    assert off[0].profile_read(off[0].PROF_MATERIALISE)[1] == 0
    assert on[0].frame_fusion_count() == off[0].frame_fusion_count() == 5
    _close(on, off)


def test_survivors_against_the_cpu_specification_without_settle(orc):
    """K = 5 frames with the switch on and no view call, then map_rows of 64 slots (read through the pending gather: survivors
    only, no settle) against orc_ekf_update along the ancestry of those slots.  Poses and gather indices of the five frames are
    those of the switch-off session (today's path), the rows are the specification's."""
    w = _world()
    B = w["B"]
    on, off = _session(True), _session(False)
    K = 5
    anc, pose = [], []
    for f in range(K):
        for eng, ses in (on, off):
            _step(eng, ses, w["fr"][f])
        off[0].sync()
        v = off[1].device_view()
        anc.append(_tensor(v["anc"]).cpu().numpy())
        pose.append(_tensor(v["pose"]).cpu().numpy())
    sel = np.unique(np.concatenate([np.random.default_rng(5).integers(0, N, 56), [0, 1, 2, 3, N - 4, N - 3, N - 2, N - 1]])).astype(np.int32)
    got = on[1].map_rows(sel)
    assert on[0].profile_read(on[0].PROF_MATERIALISE)[1] == K - 1, "a settle ran: the read was not through the survivors alone"
    part = [None] * K                                   # part[f]: the particles of frame f the chosen slots descend from
    part[K - 1] = anc[K - 1][sel]
    for f in range(K - 2, -1, -1):
        part[f] = anc[f][part[f + 1]]
    rows = np.ascontiguousarray(w["m0_host"][part[0]])  # frame 0 has no gather: particle p starts from row p
    for f in range(K):
        fr = w["fr"][f]
        if f:
            rows = np.ascontiguousarray(rows)
        out = np.full_like(rows, -777.0)
        ll = np.empty(len(sel), np.float32)
        p = pose[f][:, part[f]]
        orc.lib().orc_ekf_update(rows, out, 5 * LP, LP, L, p[0].copy(), p[1].copy(), p[2].copy(), None, len(sel),
                                 np.ascontiguousarray(fr["ids"], np.int32), fr["zx"], fr["zy"], len(fr["ids"]), B.MEAS_VAR, ll)
        rows = out
    assert np.array_equal(bits(got), bits(rows[:, :, :L]))
    _close(on, off)


def test_saved_inputs_survive_the_next_uploads():
    """The observation tensors the engine only adopted are overwritten, the next frame's table and scan uploaded, and only then
    is the view asked for: the rows must still be those of the frame that ran."""
    w = _world()
    nan = np.float32(np.nan)
    on, off = _session(True), _session(False)
    tabs = []
    for eng, ses in (on, off):
        zx, zy = torch.full((LP,), nan, device=DEV), torch.full((LP,), nan, device=DEV)
        tabs.append((zx, zy))
        for f in range(3):
            fr = w["fr"][f + 1]
            hx, hy = np.full(LP, nan, np.float32), np.full(LP, nan, np.float32)
            hx[fr["ids"]], hy[fr["ids"]] = fr["zx"], fr["zy"]
            eng.sync()
            zx.copy_(torch.from_numpy(hx))
            zy.copy_(torch.from_numpy(hy))
            torch.cuda.synchronize()
            eng.scan_upload(fr["bx"], fr["by"])
            eng.obs_set_dev(zx, zy, L)
            ses.step(0, fr["dp"], True)
        eng.sync()
        nxt = w["fr"][5]
        eng.obs_upload(nxt["ids"], nxt["zx"], nxt["zy"], L)
        zx.fill_(3.0)
        zy.fill_(-2.0)
        torch.cuda.synchronize()
        eng.scan_upload(nxt["bx"], nxt["by"])
    _assert_same(_view_state(*on), _view_state(*off), "after the uploads")
    _close(on, off)


def _then_no_observations(eng, ses, w):
    _step(eng, ses, w["fr"][3], use_obs=False)
    _step(eng, ses, w["fr"][4])


def _then_fusion_off(eng, ses, w):
    eng.frame_fusion_set(False)
    _step(eng, ses, w["fr"][3])
    eng.frame_fusion_set(True)
    _step(eng, ses, w["fr"][4])


def _then_set_map_dev(eng, ses, w):
    p = ses.poses()
    ses.set_poses(p[0], p[1], p[2])                    # drops the pending gather: every row is a particle's now
    state = _view_state(eng, ses)
    ses.set_map_dev(w["m0"], 5 * LP, LP)
    _step(eng, ses, w["fr"][3])
    _step(eng, ses, w["fr"][4])
    return state


def _then_get_map_host(eng, ses, w):
    state = {"maps": ses.maps()}
    _step(eng, ses, w["fr"][3])
    return state


@pytest.mark.parametrize("then", [_then_no_observations, _then_fusion_off, _then_set_map_dev, _then_get_map_host])
def test_every_transition_settles(then):
    w = _world()
    res = []
    for on in (True, False):
        eng, ses = _session(on)
        for f in range(3):
            _step(eng, ses, w["fr"][f])
        mid = then(eng, ses, w) or {}
        res.append((mid, _view_state(eng, ses), _final(eng, ses)))
        _close((eng, ses))
    for a, b in zip(res[0], res[1]):
        _assert_same(a, b, then.__name__)


def test_auto_session_moves_to_split_pages_and_back():
    """dense frames -> 32 of 261 observed -> dense: the session converts to split pages and back; every move reads every row"""
    w = _world()
    res = []
    for on in (True, False):
        eng, ses = _session(on, layout="auto")
        layouts = []
        for f in range(NFRAMES):
            _step(eng, ses, w["sparse"][f] if 3 <= f < 8 else w["fr"][f])   # (frame 8: the next frame on pages that takes a sample)
            eng.sync()                                  # the sample of this frame is there when the next one looks
            layouts.append(ses.layout())
        assert layouts[0] == "split" and "split_pages" in layouts and layouts[-1] == "split", layouts
        res.append((_view_state(eng, ses), _final(eng, ses), {"layouts": np.array([len(s) for s in layouts])}))
        _close((eng, ses))
    for a, b in zip(res[0], res[1]):
        _assert_same(a, b, "auto")


@pytest.mark.parametrize("layout,ess", [("split", 0.5), ("rows", 0.0)])
def test_ineligible_sessions_never_enter_the_mode(layout, ess):
    w = _world()
    res = []
    for on in (True, False):
        eng, ses = _session(on, layout=layout, ess=ess)
        for f in range(5):
            _step(eng, ses, w["fr"][f])
        res.append((_view_state(eng, ses), _final(eng, ses)))
        assert eng.profile_read(eng.PROF_MATERIALISE)[1] == 0
        _close((eng, ses))
    for a, b in zip(res[0], res[1]):
        _assert_same(a, b, layout)


def _two_ranks(on):
    """two ranks of a sharded split session in this process, one host thread each, both on this card (the in-process
    transport, as _run_c_session_ranks of test_gpu_configs.py makes them) -> per rank: poses, maps, heaviest particle, fused
    front launches, launches of the materialise stage"""
    import threading

    w = _world()
    B, pkg = w["B"], load_package()
    world, n = 2, N - 3                                 # 4096 per rank: the sharded fused front runs
    group = pkg.LocalGroup(world)
    out, errors = [None] * world, []

    def rank_main(r):
        try:
            eng = pkg.Engine(0)
            eng.survivor_rows_set(on)
            eng.profile_enable(eng.PROF_MATERIALISE)
            eng.grid_set_dev(0, w["d_edt"], pkg.grid_meta(GRID, GRID, GRID, *w["meta"]))
            comm = pkg.Comm.local(eng, group, r)
            ses = pkg.PfSession(eng, n, L, sigma=B.SIGMA, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN, seed=SEED, map_layout="split",
                                comm=comm)
            half = slice(3 * r, 3 * r + n)                  # (overlapping shares of the one initial population)
            ses.set_poses(*[p[half] for p in w["poses"]])
            ses.set_map(np.ascontiguousarray(w["m0_host"][half, :, :L]))
            for f in range(5):
                _step(eng, ses, w["fr"][f])
            res = {"poses": ses.poses(), "maps": ses.maps(), "best": np.concatenate([np.ravel(p) for p in ses.best()]),
                   "fused": np.array([eng.frame_fusion_count()]), "rows": np.array([ses.rows_received()])}
            res["materialise"] = np.array([eng.profile_read(eng.PROF_MATERIALISE)[1]])
            out[r] = res
            ses.close()
            comm.close()
            eng.close()
        except BaseException as exc:   # noqa: BLE001 - re-raised below
            errors.append((r, exc))
            try:
                comm.abort()
            except Exception:   # noqa: BLE001
                pass

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    group.close()
    if errors:
        raise errors[0][1]
    return out


def test_sharded_ranks_on_one_card_never_enter_the_mode():
    on, off = _two_ranks(True), _two_ranks(False)
    for r, (p, q) in enumerate(zip(on, off)):
        _assert_same(p, q, f"rank {r}")
        assert p["materialise"][0] == 0 and p["fused"][0] >= 3, (p["materialise"], p["fused"])
