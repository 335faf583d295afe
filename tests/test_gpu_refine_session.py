"""Scan-match refinement inside the particle-filter session (slam_pf_refine_set): the session against the same frames chained
from the stage entry points, every map layout, the resample gate, two ranks on the in-process transport, the fused-front
counter, and the host program's --refine switch."""
import json
import subprocess
import threading

import numpy as np
import pytest
import torch

import _shard_worker as W
from __graft_entry__ import PKG_DIR, load_package
from conftest import GOLDEN, bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, L, FRAMES = 2048, 64, 6
STEPS, SWEEPS = (0.05, 0.008727), 2
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
DP = [0.01, -0.005, 0.002]


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def world():
    meta, edt, bx, by, lm = W.make_world(L=L)
    x, y, th, mp = W.init_state(N, L, lm)
    return dict(meta=meta, edt=torch.from_numpy(edt).to(DEV), bx=bx, by=by, lm=lm, x=x, y=y, th=th, mp=mp)


def _engine(world):
    pkg = load_package()
    m = world["meta"]
    e = pkg.Engine(0)
    e.grid_set_dev(0, world["edt"], pkg.grid_meta(m.rows, m.cols, m.ld, m.pixel, m.min_x, m.min_y))
    e.scan_upload(world["bx"], world["by"])
    return e


def _run_session(world, layout="rows", ess=0.0, refine=True, frames=FRAMES, rank=0, ranks=1, group=None, eng=None):
    """One session (or one rank of `ranks`) over the frames, observations on in every frame -> its results"""
    pkg = load_package()
    e = eng or _engine(world)
    comm = pkg.Comm.local(e, group, rank) if group else None
    n = N // ranks
    ses = pkg.PfSession(e, n, L, comm=comm, resample_ess_frac=ess, map_layout=layout, **KW)
    if refine:
        ses.refine_set(STEPS[0], STEPS[1], SWEEPS)
    sl = slice(rank * n, (rank + 1) * n)
    ses.set_poses(world["x"][sl], world["y"][sl], world["th"][sl])
    ses.set_map(world["mp"][sl])
    fused0 = e.frame_fusion_count()
    views = []
    for f in range(frames):
        e.obs_upload(*W.observations(world["lm"], f), L)
        ses.step(0, DP, True)
        v = ses.device_view()
        e.sync()
        views.append((np.array(torch.as_tensor(v["score"], device=DEV).cpu()), np.array(torch.as_tensor(v["logw"], device=DEV).cpu())))
    out = dict(pose=ses.poses(), map=ses.maps(), views=views, best=ses.best(), mean=ses.mean(0.05), fused=e.frame_fusion_count() - fused0,
               resampled=ses.frames_resampled())
    ses.close()
    if comm:
        comm.close()
    if eng is None:
        e.close()
    return out


@pytest.fixture(scope="module")
def rows_session(world):
    return _run_session(world)


def test_refining_session_equals_the_chained_stage_calls(world, rows_session):
    """motion + refine, the landmark update on the REFINED poses, weights, resample — frame by frame from the stage entry
    points, bit for bit against the session: poses, maps, view.score and view.logw."""
    e = _engine(world)
    src = tuple(dev(world[k]) for k in ("x", "y", "th"))
    dst = tuple(torch.empty(N, device=DEV) for _ in range(3))
    maps = [dev(world["mp"]), torch.empty((N, 5, L), device=DEV)]
    anc = [None, torch.empty(N, device=DEV, dtype=torch.int32), torch.empty(N, device=DEV, dtype=torch.int32)]
    score, logw = torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    count = torch.empty(N, device=DEV, dtype=torch.int32)
    pending = None
    for f in range(FRAMES):
        e.obs_upload(*W.observations(world["lm"], f), L)
        e.motion_refine_dev(0, src, pending, dst, N, 0, DP, KW["sigma"], KW["seed"], f, STEPS[0], STEPS[1], SWEEPS, score, count)
        e.ekf_update_dev(maps[0], maps[1], 5 * L, L, L, dst[0], dst[1], dst[2], pending, N, KW["meas_var"], None)
        e.logweight_ekf_dev(score, KW["score_gain"], N, logw, None)
        e.quantise_scan_dev(logw, None, N, None)
        nxt = anc[1 + f % 2]
        e.ancestors_from_scan_dev(N, KW["seed"], f, nxt)
        got_score, got_logw = rows_session["views"][f]
        assert np.array_equal(bits(got_score), bits(host(score))), f"frame {f}: score"
        assert np.array_equal(bits(got_logw), bits(host(logw))), f"frame {f}: logw"
        src, dst, maps, pending = dst, src, maps[::-1], nxt
    a = host(pending).astype(np.int64)
    pose = np.stack([host(t)[a] for t in src])
    assert np.array_equal(bits(pose), bits(rows_session["pose"]))
    assert np.array_equal(bits(host(maps[0])[a]), bits(rows_session["map"]))
    e.close()


def test_refinement_changes_the_session(world, rows_session):
    plain = _run_session(world, refine=False)
    assert not np.array_equal(bits(plain["pose"]), bits(rows_session["pose"]))
    # every particle is weighted at a pose that scores no worse than its motion sample: frame 0 starts from the same population
    assert np.all(rows_session["views"][0][0] <= plain["views"][0][0])


@pytest.mark.parametrize("layout,ess", [("split", 0.0), ("pages", 0.0), ("split_pages", 0.0), ("rows", 0.5), ("split", 0.5),
                                        ("pages", 0.5), ("split_pages", 0.5), ("auto", 0.0)])
def test_every_layout_and_the_gate_give_the_rows_session(world, rows_session, layout, ess):
    """... identical poses and maps to the rows session.  With 64 landmarks observed in every frame the weights are so peaked
    that the effective sample size never reaches half the population: the gated sessions take the gate's path (verdict on the
    device, the host looking at it one frame behind) and resample in every frame, so they too equal the UNGATED rows session."""
    got = _run_session(world, layout, ess)
    print(f"{layout} ess={ess}: frames resampled (as far as the host has looked) {got['resampled']} of {FRAMES}")
    assert np.array_equal(bits(got["pose"]), bits(rows_session["pose"]))
    assert np.array_equal(bits(got["map"]), bits(rows_session["map"]))
    assert np.array_equal(bits(got["mean"]), bits(rows_session["mean"])) and got["best"][2] == rows_session["best"][2]


def test_fused_front_stays_off_while_refining(world):
    """A session that fuses its front launch (rows, 5 000 particles x 300 landmarks) stops doing so while it refines and
    starts again after slam_pf_refine_set(pf, 0, 0, 0)."""
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
        before = e.frame_fusion_count()
        for f in range(k0, k0 + 3):
            z = lm + 0.01 * np.float32(f)
            e.obs_upload(np.arange(Lb, dtype=np.int32), z[:, 0].copy(), z[:, 1].copy(), Lb)
            ses.step(0, DP, True)
        e.sync()
        return e.frame_fusion_count() - before

    assert frames(0) == 2          # (frame 0 has no pending gather: the front fuses from frame 1 on)
    ses.refine_set(STEPS[0], STEPS[1], SWEEPS)
    assert frames(3) == 0
    ses.refine_set(0.0, 0.0, 0)
    assert frames(6) == 3
    with pytest.raises(pkg.SlamError):
        ses.refine_set(0.05, 0.01, 17)
    with pytest.raises(pkg.SlamError):
        ses.refine_set(-0.05, 0.01, 1)
    ses.close()
    e.close()


@pytest.mark.parametrize("layout", ["rows", "split"])
def test_two_ranks_equal_one_session(world, rows_session, layout):
    """Two ranks of 1 024 particles on this card (threads of one process, in-process transport) against one session of 2 048."""
    pkg = load_package()
    group = pkg.LocalGroup(2)
    out, errors = [None, None], []

    def rank_main(r):
        try:
            out[r] = _run_session(world, layout, rank=r, ranks=2, group=group)
        except BaseException as exc:   # noqa: BLE001 - re-raised below
            errors.append(exc)

    ths = [threading.Thread(target=rank_main, args=(r,)) for r in range(2)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    group.close()
    if errors:
        raise errors[0]
    assert np.array_equal(bits(np.concatenate([o["pose"] for o in out], axis=1)), bits(rows_session["pose"]))
    assert np.array_equal(bits(np.concatenate([o["map"] for o in out], axis=0)), bits(rows_session["map"]))
    for o in out:
        assert np.array_equal(bits(o["mean"]), bits(rows_session["mean"]))
        assert o["best"][2] == rows_session["best"][2] and np.array_equal(bits(o["best"][0]), bits(rows_session["best"][0]))


def test_host_program_refine_switch(orc, tmp_path):
    """slam_pf_main ... 256 1 mean --refine 2 on the generated parity dataset completes, and its mean-pose log differs from
    the run without --refine.  The distance of both runs to the reference trajectory at the last frame is printed (for
    profiles/refine.md): a measurement, not a threshold."""
    info = json.loads((GOLDEN / "datasets.json").read_text())["parity"]
    csv = tmp_path / "parity.csv"
    orc.run_tool("gen_dataset", csv, *info["gen_args"])
    exe = PKG_DIR / "lib" / "slam_pf_main"
    ref = np.array([[float(v) for v in ln.split("=")[1].split()] for ln in (GOLDEN / "parity_pose.txt").read_text().splitlines()])
    logs = []
    for extra in ([], ["--refine", "2"]):
        r = subprocess.run([str(exe), str(csv), "1000", "1079", str(tmp_path / "map.csv"), "256", "1", "mean", *extra], check=True,
                           capture_output=True, text=True)
        poses = [ln for ln in r.stdout.splitlines() if ln.startswith("pose =")]
        assert len(poses) == 999
        got = np.array([[float(v) for v in ln.split("=")[1].split()] for ln in poses])
        d = np.hypot(got[:, 0] - ref[:, 0], got[:, 1] - ref[:, 1])
        print(f"slam_pf_main 256 particles {' '.join(extra) or '(no refinement)'}: distance to the reference trajectory at the last frame "
              f"{d[-1]:.4f} m (max over the run {d.max():.4f} m), |dtheta| at the last frame {abs(got[-1, 2] - ref[-1, 2]):.5f} rad; "
              f"{r.stderr.strip()}")
        logs.append(poses)
    assert logs[0] != logs[1]
    # the usage line names the switch
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 2 and "--refine SWEEPS" in r.stderr
