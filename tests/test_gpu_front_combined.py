"""One workgroup scores AND updates its 64 particles and makes their log-weights (csrc/front_kernels.hip:
frame_particle_kernel; score_body.h: score_stage / STAGED; ekf_split_body.h: ekf_split_group / kPosesStaged;
scan_kernels.hip: quantise_scan_cov_kernel): a survivor-rows frame of the split layout with 8 particles per wavefront then
has no weights' launch, and the covariance classes' update rides in the scan's launch.  Not a bit may change.

The comparison partner is the same session with frame_fusion_set(False) — the separate launches, which
tests/test_gpu_front_diet.py and tests/test_gpu_frame_front_at_size.py pin to the CPU specification — compared as bit
patterns after every frame: poses, the pending ancestor index (it pins the log-weights and their maximum through the integer
CDF), best() and mean(), the landmark rows of every particle, the classes and their covariance rows.

Which kernel ran: a frame whose front launch made the weights has no launch in the SLAM_PROF_WEIGHTS bracket (timing that
bracket does not split the front launch; only SLAM_PROF_SCORE does), every other frame has one.

Shapes: n = 4099 / 4127 (the last workgroup of 64 holds 3 / 31 particles: partial groups and wavefronts without a group),
n = 4096 (exact); L = 261 (plane stride 288: a partial second pass) and L = 129 (the shortest row the front launch takes);
360 beams and 7 (fewer than one pipeline round); the packed byte grid and a float grid that does not pack; n = 16 835 for the
workgroups that run the update before the score (blockIdx.x >= 256), the last, partial one among them.  World and maps
follow tests/test_gpu_survivor_rows.py: several dozen covariance classes, landmarks nobody has seen yet (first sightings),
frames 2 and 4 with unobserved landmarks (NaN in the table), frame 4 with a whole batch of them.
PARITY UNPINNED: the reference has no landmarks.
"""
import functools

import numpy as np
import pytest
import torch

from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
GRID, SEED, FRAMES = 1024, 1234, 6


def _tensor(a):
    return torch.as_tensor(a, device=DEV)


@functools.lru_cache(maxsize=None)
def _edt(grid):
    """bench.py's room as the engine's EDT ("packed") or with every cell scaled a little ("float": not the square root of an
    integer any more, so the grid does not pack); made once"""
    import bench as B

    pixel, min_x, min_y = np.float32(20.48 / GRID), np.float32(-4.24), np.float32(-10.24)
    occ = B.occupancy(GRID, float(pixel), float(min_x), float(min_y))
    eng = load_package().Engine(0)
    d_edt = torch.empty((GRID, GRID), dtype=torch.float32, device=DEV)
    eng.edt_dev(torch.from_numpy(occ).to(DEV), GRID, GRID, GRID, 10.0, d_edt)
    eng.sync()
    eng.close()
    if grid == "float":
        g = torch.Generator(device="cpu").manual_seed(11)
        d_edt = d_edt * (0.9 + 0.2 * torch.rand((GRID, GRID), generator=g)).to(DEV)
    return d_edt, (pixel, min_x, min_y)


@functools.lru_cache(maxsize=None)
def _world(n, L, beams):
    """frames, initial poses and maps (the recipe of test_gpu_survivor_rows._world at these sizes); made once, never changed"""
    import bench as B

    LP = (L + 31) // 32 * 32
    rng = np.random.default_rng(4321)
    landmarks = B.make_landmarks(L, rng)
    fr = B.make_frames(FRAMES, beams, landmarks, rng, 0)
    for f in (2, 4):   # some landmarks unobserved (NaN in the table), in frame 4 a whole batch of 128 among them
        gone = [np.arange(7, L, 5)] + ([np.arange(128, 256)] if f == 4 else [])
        keep = ~np.isin(fr[f]["ids"], np.concatenate(gone))
        fr[f] = dict(fr[f], ids=fr[f]["ids"][keep], zx=fr[f]["zx"][keep], zy=fr[f]["zy"][keep])
    g = torch.Generator(device="cpu").manual_seed(SEED)
    p0 = B.true_pose(0)
    poses = [(p0[k] + s * torch.randn(n, generator=g)).numpy().astype(np.float32) for k, s in ((0, 0.05), (1, 0.05), (2, 0.01))]
    m0 = torch.zeros((n, 5, LP), dtype=torch.float32, device=DEV)
    torch.manual_seed(7)
    B.fill_maps(torch, m0, landmarks, L, DEV, n)
    fam = torch.zeros(n, dtype=torch.long)   # runs of 1 .. 96 neighbouring particles share their covariances: the classes
    i, frng = 0, np.random.default_rng(3)
    while i < n:
        k = int(frng.integers(1, 97))
        fam[i:i + k] = i
        i += k
    a = 0.2 * torch.randn((n, 4, L), device=DEV)
    m0[:, 2, :L] = a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + 0.02
    m0[:, 3, :L] = a[:, 0] * a[:, 2] + a[:, 1] * a[:, 3]
    m0[:, 4, :L] = a[:, 2] * a[:, 2] + a[:, 3] * a[:, 3] + 0.02
    m0[:, 2, 5:L:17] = -1.0                   # first sightings
    m0[:, 2:5] = m0[fam.to(DEV), 2:5]
    torch.cuda.synchronize()
    return dict(B=B, fr=fr, poses=poses, m0=m0, L=L, LP=LP, n=n, true=np.array(p0, np.float32))


def _session(w, grid, fused, sigma=None, poses=None, m0=None):
    B, pkg = w["B"], load_package()
    d_edt, meta = _edt(grid)
    eng = pkg.Engine(0)
    eng.frame_fusion_set(fused)
    eng.profile_enable(eng.PROF_WEIGHTS)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(GRID, GRID, GRID, *meta))
    ses = pkg.PfSession(eng, w["n"], w["L"], sigma=B.SIGMA if sigma is None else sigma, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN,
                        seed=SEED, map_layout="split", resample_ess_frac=0.0)
    ses.set_poses(*(w["poses"] if poses is None else poses))
    ses.set_map_dev(w["m0"] if m0 is None else m0, 5 * w["LP"], w["LP"])
    eng.sync()
    assert ses.layout() == "split"
    return eng, ses


def _step(eng, ses, w, f, use_obs=True):
    """-> (fused front launches, weights' launches) of the frame"""
    fr = w["fr"][f]
    fused_before = eng.frame_fusion_count()
    eng.scan_upload(fr["bx"], fr["by"])
    eng.obs_upload(fr["ids"], fr["zx"], fr["zy"], w["L"])
    ses.step(0, fr["dp"], use_obs)
    eng.sync()
    return eng.frame_fusion_count() - fused_before, eng.profile_read(eng.PROF_WEIGHTS)[1]


def _state(eng, ses, w):
    """what a frame left (asking for the views settles the rows of a survivor-rows frame)"""
    n = w["n"]
    v = ses.device_view()
    out = {k: _tensor(v[k]).cpu().numpy() for k in ("pose", "anc", "logw", "score", "loglik") if v[k] is not None}
    best = ses.best()
    out["best"] = np.concatenate([np.ravel(best[0]), np.ravel(best[1])]).astype(np.float32)
    out["best_index"] = np.array([best[2]])
    out["mean"] = ses.mean(float(w["true"][2]))
    out["rows"] = ses.map_rows(np.arange(n, dtype=np.int32))
    sv = ses.split_view()
    out["cls"] = _tensor(sv["cls"])[:n].cpu().numpy()
    used = torch.from_numpy(np.unique(out["cls"])).to(DEV).long()
    out["cov"] = _tensor(sv["cov"])[used].cpu().numpy()
    out["covx"] = _tensor(sv["covx"])[used].cpu().numpy()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(bits(a[k]), bits(b[k])), f"{what}: {k}"


def _close(*pairs):
    for eng, ses in pairs:
        ses.close()
        eng.close()


def _run_pair(w, grid, observe=(True,) * FRAMES, prepare=None, frames=FRAMES, **kw):
    """the session and its partner with the separate launches, frame by frame; -> the frames whose front launch made the
    weights, and the partner's states"""
    one, two = _session(w, grid, True, **kw), _session(w, grid, False, **kw)
    made, states = [], []
    for f in range(frames):
        if prepare:
            for eng, ses in (one, two):
                prepare(f, eng, ses)
        fused, weights = _step(*one, w, f, observe[f])
        fused2, weights2 = _step(*two, w, f, observe[f])
        assert (fused2, weights2) == (0, 1), f"frame {f}: the partner did not run the separate launches"
        # the frames meant for the new kernel: fused, 8 particles per updating wavefront (the engine chooses 8 once the last
        # resample left few distinct ancestors, 4 before), four lanes per pose
        meant = fused == 1 and one[0].frame_front_last() == (8, 4)
        print(f"frame {f}: fused {fused}, front {one[0].frame_front_last()}, weights' launches {weights}")
        assert fused == (1 if f and observe[f] else 0) and weights == (0 if meant else 1), f"frame {f}: {fused} fused, {weights} weights' launches"
        if meant:
            made.append(f)
        a, b = _state(*one, w), _state(*two, w)
        _assert_same(a, b, f"frame {f}")
        states.append(b)
    _close(one, two)
    return made, states


@pytest.mark.parametrize("n,L,beams,grid", [(4099, 261, 360, "packed"), (4127, 261, 360, "float"), (4096, 261, 7, "packed"),
                                            (4099, 129, 360, "float"), (4127, 129, 7, "packed"), (4096, 129, 360, "packed"),
                                            (4099, 261, 7, "float")])
def test_same_bits_as_the_separate_launches(n, L, beams, grid):
    """six frames, resampling every frame; frames 2 and 4 with landmarks nobody observed and first sightings (SPECIAL batches)"""
    made, _ = _run_pair(_world(n, L, beams), grid)
    # (frame 0 has no resample index yet: no fused front; later a frame may come with 4 particles per wavefront — the engine goes by
    # the last resample's count of distinct ancestors, read without waiting — and then stays with the kernels it had: _run_pair
    # has checked frame by frame that the new kernel ran exactly where the launch was (8, 4))
    assert set(made) <= set(range(1, FRAMES)) and len(made) >= 3, made


def test_a_frame_without_observations_between_two_with():
    """frame 3 has no landmark update: no fused front, the separate launches — and the frames around it are combined again"""
    observe = (True, True, True, False, True, True)
    made, _ = _run_pair(_world(4099, 261, 360), "packed", observe)
    assert 3 not in made and any(f < 3 for f in made) and any(f > 3 for f in made), made


def test_one_particle_of_the_last_workgroup_carries_the_maximum():
    """before frame 1 every ancestor but the last particle's is moved 1.5 m off: the frame's maximum log-weight then lies with
    a particle of the last, partial workgroup (3 of 64), alone"""
    w = _world(4099, 261, 360)
    n = w["n"]
    where = {}

    def prepare(f, eng, ses):
        if f != 1:
            return
        v = ses.device_view()
        anc = _tensor(v["anc"]).cpu().numpy()
        a = int(anc[n - 1])
        assert a not in anc[:n // 64 * 64], "the last particle's ancestor has offspring in a full workgroup"
        pose = _tensor(v["pose"])
        keep = pose[:, a].clone()
        pose[0] += 1.5
        pose[1] += 1.5
        pose[:, a] = keep
        torch.cuda.synchronize()
        where["a"] = a

    made, states = _run_pair(w, "packed", prepare=prepare)
    assert 1 in made, made
    lw = states[1]["logw"][:n]
    top = int(np.argmax(lw))
    assert top >= n // 64 * 64 and np.sum(lw == lw[top]) == 1, (top, lw[top])
    assert lw[top] - np.max(lw[:n // 64 * 64]) > 10.0, "the moved particles are not clearly worse"


def test_all_weights_equal():
    """No motion noise, one pose, one map: every particle has the same weight.  Every particle is then its own ancestor, the
    engine keeps 4 particles per updating wavefront and such a frame stays with the kernels it had (frames 0, 1 and from 3 on).
    To meet equal weights in the NEW kernel, all ancestors but three are moved far off before frame 1: its resample keeps the
    offspring of the three alone — few distinct ancestors, so frame 2 runs 8 particles per wavefront —, and in frame 2 every
    particle descends from bit-identical ancestors without noise: all weights equal, the block maxima and the `lw > m` rule
    meet equal values in every workgroup, the last, partial one included."""
    w = _world(4127, 261, 360)
    n = w["n"]
    poses = [np.full(n, p[0], np.float32) for p in w["poses"]]
    m0 = w["m0"][:1].expand(n, -1, -1).contiguous()
    kept = torch.tensor([5, 2000, n - 2], device=DEV)

    def prepare(f, eng, ses):
        if f != 1:
            return
        pose = _tensor(ses.device_view()["pose"])   # (the pending ancestor index is the identity here: equal weights)
        keep = pose[:, kept].clone()
        pose[0] += 3.0
        pose[1] += 3.0
        pose[2] += 0.5
        pose[:, kept] = keep
        torch.cuda.synchronize()

    made, states = _run_pair(w, "packed", prepare=prepare, sigma=(0.0, 0.0, 0.0), poses=poses, m0=m0)
    lw1 = states[1]["logw"][:n]
    others = np.setdiff1d(np.arange(n), kept.cpu().numpy())
    assert np.min(lw1[kept.cpu().numpy()]) - np.max(lw1[others]) > 40.0, "the moved particles may still leave offspring"
    assert set(np.unique(states[1]["anc"][:n])) <= set(kept.cpu().numpy().tolist()), "a moved particle left offspring"
    assert 2 in made and 0 not in made and 1 not in made, made
    for f, s in enumerate(states):
        if f == 1:
            continue
        lw = s["logw"][:n]
        assert np.all(bits(lw) == bits(lw)[0]), f"frame {f}: the log-weights differ"


def test_the_workgroups_that_update_before_they_score():
    """n = 16 835: 264 workgroups of 64, 33 per XCD, so blockIdx.x reaches 256 .. 263 — the workgroups that run the update before
    the score — and the last, partial workgroup (3 particles) is one of them (particles from 64 * 263 on: XCD 7, the 33rd there)"""
    n = 263 * 64 + 3
    made, _ = _run_pair(_world(n, 129, 360), "packed", frames=3)
    assert made and set(made) <= {1, 2}, made   # (which of the two come as (8, 4) is the engine's choice: _run_pair)
