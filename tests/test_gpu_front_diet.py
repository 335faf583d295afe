"""The fused front launch after its diet (csrc/ekf_split_body.h, score_body.h, ekf_wave.h, ekf_math.h): one wavefront per
workgroup makes the workgroup's motion samples and hands them over in LDS behind a barrier — in the updating workgroups and
in the scoring ones with four lanes per pose —, the group's log-likelihood sums are reduced on the halving schedule, and the
likelihood term starts from the negated product.  None of it may change a bit.

The comparison partner is the CPU specification DIRECTLY (orc_motion_sample, orc_score_poses_det, orc_ekf_update), every
particle, every frame, as tests/test_gpu_frame_front_at_size.py compares at bench.py's sizes; here at the smallest shapes at
which the fused front still runs and every tail of the new hand-over is partial:
  n = 4099: a last group of 3 particles, the last updating workgroup (32 particles at 8 per wavefront) with one wavefront of
            3 particles and three empty ones behind the barrier, the last scoring workgroup (64 poses) with 3 poses;
  n = 4127: a last group of 7, a last updating workgroup of 31 particles (7 in its last wavefront; at 4 per wavefront: 3 in
            the last of four), a last scoring workgroup with 31 poses;
  L = 261 : plane stride 288, a partial second pass of 256 landmarks.
World, maps and frames are those of tests/test_gpu_survivor_rows.py (bench.py's room; several dozen covariance classes,
landmarks nobody has seen yet, frames 2 and 4 with unobserved landmarks, frame 4 with a whole batch of them).  The engine
chooses the particles per updating wavefront itself — split: 8 once the resample stage has reported few distinct ancestors
(here from the first fused frame on), 4 before; rows: 2, then 4 — and slam_frame_front_last says which ran;
slam_ekf_form_set(1) / (2) holds it to 4 / 2 on the split layout, so all three group sizes of the split launch run.
PARITY UNPINNED: the reference has no landmarks.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_survivor_rows as S
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_frame_front_at_size import _rows_of, _tensor

pytestmark = pytest.mark.gpu
DEV = S.DEV
L, LP = S.L, S.LP
FRAMES = 6


@functools.lru_cache(maxsize=None)
def _world(n):
    """the recipe of test_gpu_survivor_rows._world for a population of n (its module constant N is 4099); made once per n"""
    old = S.N
    S.N = n
    try:
        w = S._world.__wrapped__()
    finally:
        S.N = old
    pixel, min_x, min_y = w["meta"]
    w["edt"] = w["d_edt"].cpu().numpy()
    w["ometa_args"] = (S.GRID, S.GRID, S.GRID, float(pixel), float(min_x), float(min_y))
    return w


def _session(w, n, layout, survivor_rows, form):
    B, pkg = w["B"], load_package()
    eng = pkg.Engine(0)
    eng.ekf_form_set(form)
    eng.survivor_rows_set(survivor_rows)
    eng.profile_enable(eng.PROF_MATERIALISE)
    eng.grid_set_dev(0, w["d_edt"], pkg.grid_meta(S.GRID, S.GRID, S.GRID, *w["meta"]))
    ses = pkg.PfSession(eng, n, L, sigma=B.SIGMA, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN, seed=S.SEED, map_layout=layout,
                        resample_ess_frac=0.0)
    ses.set_poses(*w["poses"])
    ses.set_map_dev(w["m0"], 5 * LP, LP)
    eng.sync()
    assert ses.layout() == layout
    return eng, ses


@pytest.mark.parametrize("layout,survivor_rows,form", [("split", True, -1), ("split", False, -1), ("split", True, 1), ("split", True, 2), ("rows", False, -1)])
@pytest.mark.parametrize("n", [4099, 4127])
def test_every_particle_against_the_cpu_specification(orc, n, layout, survivor_rows, form):
    w = _world(n)
    B = w["B"]
    ometa = orc.meta(*w["ometa_args"])
    eng, ses = _session(w, n, layout, survivor_rows, form)
    every = torch.arange(n, device=DEV)
    ran = set()
    for f in range(FRAMES):
        fr = w["fr"][f]
        v = ses.device_view()                                      # (asks for the views: a survivor-rows session settles)
        anc = None if v["anc"] is None else _tensor(v["anc"]).cpu().numpy()
        src_pose = _tensor(v["pose"]).cpu().numpy()
        src_rows = every if anc is None else torch.from_numpy(anc).to(DEV)
        prior = _rows_of(ses, layout, src_rows).cpu().numpy()     # [n][5][LP]: the ancestors' rows BEFORE the step
        fused_before = eng.frame_fusion_count()
        S._step(eng, ses, fr)
        eng.sync()
        assert eng.frame_fusion_count() - fused_before == (1 if f else 0), f"frame {f}: the front was not one fused launch"
        if f:
            ran.add(eng.frame_front_last())
        v = ses.device_view()
        pose = _tensor(v["pose"]).cpu().numpy()
        x, y, th = orc.motion_sample(src_pose[0], src_pose[1], src_pose[2], anc, n, 0, fr["dp"], np.array(B.SIGMA, np.float32),
                                     S.SEED, f)
        assert np.array_equal(bits(pose), bits(np.stack([x, y, th]))), f"frame {f}: poses"
        want_score, want_count = orc.score_poses_det(ometa, w["edt"], fr["bx"], fr["by"], x, y, th)
        assert np.array_equal(_tensor(v["count"]).cpu().numpy()[:n], want_count), f"frame {f}: in-bounds counts"
        assert np.array_equal(bits(_tensor(v["score"]).cpu().numpy()[:n]), bits(want_score)), f"frame {f}: scores"
        want = np.full_like(prior, -777.0)
        want_ll = np.empty(n, np.float32)
        orc.lib().orc_ekf_update(np.ascontiguousarray(prior), want, 5 * LP, LP, L, x.copy(), y.copy(), th.copy(), None, n,
                                 np.ascontiguousarray(fr["ids"], np.int32), fr["zx"], fr["zy"], len(fr["ids"]), B.MEAS_VAR, want_ll)
        got_ll = _tensor(v["loglik"]).cpu().numpy()[:n]
        assert np.array_equal(bits(got_ll), bits(want_ll)), f"frame {f}: log-likelihoods"
        got = _rows_of(ses, layout, every).cpu().numpy()          # the rows along the ancestry: this frame's from the last one's
        assert np.array_equal(bits(got[:, :, :L]), bits(want[:, :, :L])), f"frame {f}: landmark rows"
    if layout == "split":
        groups = {g for g, _ in ran}
        assert (groups == {2} if form == 2 else groups == {4} if form == 1 else 8 in groups and groups <= {4, 8}), ran
        assert {q for _, q in ran} == {4}, ran
        # launch structure as before: a survivor frame's rows come from the launch behind its resample + one settle per view
        assert eng.profile_read(eng.PROF_MATERIALISE)[1] == (2 * (FRAMES - 1) if survivor_rows else 0)
    else:
        assert {g for g, _ in ran} <= {2, 4} and {q for _, q in ran} == {4}, ran
    S._close((eng, ses))


def test_two_ranks_on_one_card_equal_one_rank():
    """a sharded split session, 2 x 4099 x 261 (threads, in-process transport): its fused front goes out in two launches, each
    leaving out some groups (group_filter) whose wavefronts still have to meet the workgroup's barrier"""
    from test_gpu_configs import _run_c_session_ranks

    n = 4099
    one = _run_c_session_ranks(1, 2 * n, L, FRAMES, transport=None, layout="split")[0]
    two = _run_c_session_ranks(2, 2 * n, L, FRAMES, layout="split")
    assert all(p["fused"] >= FRAMES - 3 for p in two), [p["fused"] for p in two]
    assert sum(sum(p["rows"]) for p in two) > 0, "nothing migrated"
    assert np.array_equal(bits(np.concatenate([p["pose"] for p in two], axis=1)), bits(one["pose"]))
    assert np.array_equal(bits(np.concatenate([p["map"] for p in two], axis=0)), bits(one["map"]))
    for p in two:
        assert p["best"][1] == one["best"][1] and p["best"][2] == one["best"][2]
        assert np.array_equal(bits(p["best"][0]), bits(one["best"][0]))
