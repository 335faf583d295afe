#!/usr/bin/env python3
"""profiles/assoc_measure.py [N L ROUNDS REPS] — data association on the GPU, through the package, in ONE process:
  * slam_associate_dev (SLAM_PROF_PAGES) for K = 8, 32 and 64 detections, out of place through resampled ancestors;
  * slam_ekf_update_assoc_dev (SLAM_PROF_EKF) under the table the K = 64 launch wrote, beside slam_ekf_update_dev
    (slam_ekf_form_set(e, 0): the one-wavefront-per-particle kernel, the code both share) fed an observation table of the
    same 64 landmarks, alternated in blocks of REPS launches for ROUNDS rounds after a warm-up of each.
Per kernel the median, minimum and maximum over the rounds of the mean launch time.  The scene: L landmarks on a 40 m square,
10 % of every map not seen yet, the particles within centimetres of one pose, the detections observations of landmarks of
the scene from that pose.  Measurement tooling: prints, asserts nothing about time.  Default: 65 536 x 500 (plane stride 512),
6 rounds of 10 launches."""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "6", "10"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, Q, GATE, NEW_GATE = "cuda:0", 0.02, 9.21, 50.0
pkg = load_package()
e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
lm = rng.uniform(-20, 20, (L, 2)).astype(np.float32)
x, y, th = (torch.as_tensor((s * rng.standard_normal(n)).astype(np.float32)).to(DEV) for s in (0.05, 0.05, 0.002))
# resampled ancestors: ~6 % distinct, the offspring of one ancestor neighbours (what a systematic resample leaves)
heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
d_in = torch.empty((n, 5, Lp), device=DEV)
d_in[:, 0, :L] = torch.as_tensor(lm[:, 0]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 1, :L] = torch.as_tensor(lm[:, 1]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 2], d_in[:, 3], d_in[:, 4] = 0.05, 0.01, 0.04
d_in[:, 2, :L][torch.rand((n, L), device=DEV) < 0.1] = -1.0
d_in[:, :, L:] = 0.0
d_out = torch.empty((n, 5, Lp), device=DEV)
d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_stats = torch.empty((n, 3), dtype=torch.int32, device=DEV)
ids = np.sort(rng.permutation(L)[:64]).astype(np.int32)
order = rng.permutation(64)


def detections(K):
    return lm[ids[order[:K]], 0].copy(), lm[ids[order[:K]], 1].copy()   # (the pose is the origin, heading 0: z = m)


def associate():
    e.associate_dev(d_in, 5 * Lp, Lp, L, x, y, th, anc, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, d_stats)


def timed(call, kernel):
    out = []
    for _ in range(rounds):
        for _ in range(reps):
            call()
        e.sync()
        ms, launches = e.profile_read(kernel)
        assert launches == reps
        out.append(1e3 * ms / launches)
    return out


def report(name, t):
    print(f"  {name:58s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us")
    return statistics.median(t)


print(f"{n} x {L} (plane stride {Lp}), {len(heads)} distinct ancestors; {rounds} rounds x {reps} launches")
for K in (8, 32, 64):
    e.detections_upload(*detections(K))
    for _ in range(5):
        associate()
    e.sync()
    e.profile_enable(pkg.Engine.PROF_PAGES)
    t = timed(associate, pkg.Engine.PROF_PAGES)
    e.profile_enable()
    st = d_stats.sum(dim=0).cpu().numpy() / n
    report(f"associate_kernel K = {K}", t)
    print(f"      per particle: matched {st[0]:.2f}  created {st[1]:.2f}  dropped {st[2]:.2f}")

# the table of K = 64 is in d_assoc; the observation table that names the same landmarks
zx, zy = detections(64)
e.obs_upload(ids[order], zx, zy, L)
e.ekf_form_set(0)
calls = {
    "slam_ekf_update_dev, form 0, 64 of the landmarks observed": lambda: e.ekf_update_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, Q, None),
    "slam_ekf_update_assoc_dev under the K = 64 table": lambda: e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, Q, d_assoc, Lp, None),
}
for call in calls.values():
    for _ in range(5):
        call()
e.sync()
e.profile_enable(pkg.Engine.PROF_EKF)
times = {k: [] for k in calls}
for _ in range(rounds):
    for name, call in calls.items():
        for _ in range(reps):
            call()
        e.sync()
        ms, launches = e.profile_read(pkg.Engine.PROF_EKF)
        assert launches == reps
        times[name].append(1e3 * ms / launches)
e.profile_enable()
a, b = (report(name, t) for name, t in times.items())
print(f"  ratio assoc update / plain update (medians): {b / a:.3f}")
e.close()
