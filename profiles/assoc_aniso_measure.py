#!/usr/bin/env python3
"""profiles/assoc_aniso_measure.py [N L K ROUNDS REPS] — data association under a 2x2 measurement covariance beside its isotropic
parents, through the package, in ONE process:
  * slam_associate_dev / slam_associate_aniso_dev (SLAM_PROF_PAGES), K detections, out of place through resampled ancestors,
    alternated in blocks of REPS launches for ROUNDS rounds after a warm-up of each;
  * slam_ekf_update_assoc_dev / slam_ekf_update_assoc_aniso_dev (SLAM_PROF_EKF), each under the table its own association wrote,
    alternated likewise;
  * slam_pf_step of two rows sessions (NS x L, the world of the session tests), one behind slam_pf_assoc_set and one behind
    slam_pf_assoc_cov_set, wall clock around blocks of REPS frames, alternated likewise.
Per item the median, minimum and maximum over the rounds of the mean time.  The scene of profiles/assoc_measure.py.
Measurement tooling: prints, asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), K = 24, 12 rounds of 20."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

n, L, K, rounds, reps = (int(v) for v in (sys.argv[1:6] + ["65536", "500", "24", "12", "20"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, Q, COV, GATE, NEW_GATE = "cuda:0", 0.02, (0.02, 0.012, 0.015), 9.21, 50.0
pkg = load_package()
e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
lm = rng.uniform(-20, 20, (L, 2)).astype(np.float32)
x, y, th = (torch.as_tensor((s * rng.standard_normal(n)).astype(np.float32)).to(DEV) for s in (0.05, 0.05, 0.002))
heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
d_in = torch.empty((n, 5, Lp), device=DEV)
d_in[:, 0, :L] = torch.as_tensor(lm[:, 0]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 1, :L] = torch.as_tensor(lm[:, 1]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 2], d_in[:, 3], d_in[:, 4] = 0.05, 0.01, 0.04
d_in[:, 2, :L][torch.rand((n, L), device=DEV) < 0.1] = -1.0
d_in[:, :, L:] = 0.0
d_out = torch.empty((n, 5, Lp), device=DEV)
tabs = {k: torch.empty((n, Lp), dtype=torch.uint8, device=DEV) for k in ("iso", "aniso")}
d_stats = torch.empty((n, 3), dtype=torch.int32, device=DEV)
pick = rng.permutation(L)[:K]
e.detections_upload(lm[pick, 0].copy(), lm[pick, 1].copy())   # (the pose is the origin, heading 0: z = m)
pose = (x, y, th)


def alternate(calls, kernel):
    for call in calls.values():
        for _ in range(5):
            call()
    e.sync()
    e.profile_enable(kernel)
    times = {k: [] for k in calls}
    for _ in range(rounds):
        for name, call in calls.items():
            for _ in range(reps):
                call()
            e.sync()
            ms, launches = e.profile_read(kernel)
            assert launches == reps
            times[name].append(1e3 * ms / launches)
    e.profile_enable()
    med = []
    for name, t in times.items():
        print(f"  {name:64s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us")
        med.append(statistics.median(t))
    print(f"  ratio of the medians (2x2 / isotropic): {med[1] / med[0]:.3f}   of the minima: {min(times[list(calls)[1]]) / min(times[list(calls)[0]]):.3f}")


print(f"{n} x {L} (plane stride {Lp}), K = {K}, {len(heads)} distinct ancestors; {rounds} rounds x {reps} launches")
alternate({
    "associate_kernel<create> (slam_associate_dev)": lambda: e.associate_dev(d_in, 5 * Lp, Lp, L, *pose, anc, n, Q, GATE, NEW_GATE, 1, tabs["iso"], Lp, d_stats),
    "associate_aniso_kernel<create> (slam_associate_aniso_dev)": lambda: e.associate_aniso_dev(d_in, 5 * Lp, Lp, L, *pose, anc, n, COV, GATE, NEW_GATE, 1, tabs["aniso"], Lp, d_stats),
}, pkg.Engine.PROF_PAGES)
st = d_stats.sum(dim=0).cpu().numpy() / n
print(f"      per particle (2x2): matched {st[0]:.2f}  created {st[1]:.2f}  dropped {st[2]:.2f}")
alternate({
    "table update, meas_var * I (slam_ekf_update_assoc_dev)": lambda: e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, anc, n, Q, tabs["iso"], Lp, None),
    "table update, 2x2 Q (slam_ekf_update_assoc_aniso_dev)": lambda: e.ekf_update_assoc_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, anc, n, COV, tabs["aniso"], Lp, None),
}, pkg.Engine.PROF_EKF)
e.close()
del d_in, d_out, tabs

# ---- the associating session's step, isotropic and under the new switch
import _shard_worker as W  # noqa: E402

NS, LS, KS = 16384, 500, K
meta, edt, bx, by, wlm = W.make_world(L=LS)
sx, sy, sth, mp = W.init_state(NS, LS, wlm)
mp[:, 2, LS // 2:] = -1.0
d_edt = torch.from_numpy(edt).to(DEV)
sessions = {}
for name in ("slam_pf_assoc_set", "slam_pf_assoc_cov_set"):
    eng = pkg.Engine(0)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    eng.scan_upload(bx, by)
    ses = pkg.PfSession(eng, NS, LS, seed=77, sigma=(0.02, 0.02, 0.004), meas_var=Q, score_gain=0.05, map_layout="rows")
    if name == "slam_pf_assoc_set":
        ses.assoc_set(GATE, NEW_GATE, True)
    else:
        ses.assoc_cov_set(COV, GATE, NEW_GATE, True)
    ses.set_poses(sx, sy, sth)
    ses.set_map(mp)
    sessions[name] = (eng, ses)
frame = 0


def steps(eng, ses, count):
    global frame
    for _ in range(count):
        _, zx, zy = W.observations(wlm, frame % 8)
        eng.detections_upload(zx[:KS].copy(), zy[:KS].copy())
        ses.step(0, [0.01, -0.005, 0.002], True)
        frame += 1
    eng.sync()


for eng, ses in sessions.values():
    steps(eng, ses, 5)
times = {k: [] for k in sessions}
for _ in range(rounds):
    for name, (eng, ses) in sessions.items():
        t0 = time.perf_counter()
        steps(eng, ses, reps)
        times[name].append(1e6 * (time.perf_counter() - t0) / reps)
print(f"session step, {NS} x {LS} on rows, K = {KS}, every frame resamples; wall clock per frame incl. the detections' upload, {rounds} rounds x {reps} frames")
med = []
for name, t in times.items():
    print(f"  {name:64s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us")
    med.append(statistics.median(t))
print(f"  ratio of the medians (2x2 / isotropic): {med[1] / med[0]:.3f}")
for eng, ses in sessions.values():
    ses.close()
    eng.close()
