#!/usr/bin/env python3
"""profiles/assoc_detcov_measure.py [N L ROUNDS REPS] — data association under a measurement covariance per detection beside its
2x2 twins, through the package, in ONE process, for K = 8, 32 and 64 detections:
  * slam_associate_aniso_dev / slam_associate_detcov_dev (SLAM_PROF_PAGES), out of place through resampled ancestors, alternated
    in blocks of REPS launches for ROUNDS rounds after a warm-up of each;
  * slam_ekf_update_assoc_aniso_dev / slam_ekf_update_assoc_detcov_dev (SLAM_PROF_EKF), each under the table its own association
    wrote, alternated likewise.
Per item the median, minimum and maximum over the rounds of the mean time.  The scene of profiles/assoc_measure.py; every Q_k of
the per-detection stage is the range / bearing model a_k u u^T + b_k v v^T of its detection (range_var 4e-6, bearing_var 1e-4).
Measurement tooling: prints, asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), 12 rounds of 20."""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from __graft_entry__ import load_package  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "12", "20"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, COV, GATE, NEW_GATE = "cuda:0", (0.02, 0.012, 0.015), 9.21, 50.0
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
tabs = {k: torch.empty((n, Lp), dtype=torch.uint8, device=DEV) for k in ("aniso", "detcov")}
d_stats = torch.empty((n, 3), dtype=torch.int32, device=DEV)
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
    print(f"  ratio of the medians (per detection / 2x2): {med[1] / med[0]:.3f}   of the minima: {min(times[list(calls)[1]]) / min(times[list(calls)[0]]):.3f}")


print(f"{n} x {L} (plane stride {Lp}), {len(heads)} distinct ancestors; {rounds} rounds x {reps} launches")
for K in (8, 32, 64):
    pick = rng.permutation(L)[:K]
    zx, zy = lm[pick, 0].copy(), lm[pick, 1].copy()                # (the pose is the origin, heading 0: z = m)
    r2 = zx * zx + zy * zy
    ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
    a, b = np.float32(4e-6), np.float32(1e-4) * r2
    e.detections_upload(zx, zy)
    e.detections_cov_upload(a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux)
    print(f"K = {K}")
    alternate({
        "associate_aniso_kernel<create> (slam_associate_aniso_dev)": lambda: e.associate_aniso_dev(d_in, 5 * Lp, Lp, L, *pose, anc, n, COV, GATE, NEW_GATE, 1, tabs["aniso"], Lp, d_stats),
        "associate_detcov_kernel<create> (slam_associate_detcov_dev)": lambda: e.associate_detcov_dev(d_in, 5 * Lp, Lp, L, *pose, anc, n, GATE, NEW_GATE, 1, tabs["detcov"], Lp, d_stats),
    }, pkg.Engine.PROF_PAGES)
    st = d_stats.sum(dim=0).cpu().numpy() / n
    print(f"      per particle (per detection): matched {st[0]:.2f}  created {st[1]:.2f}  dropped {st[2]:.2f}")
    alternate({
        "table update, 2x2 Q (slam_ekf_update_assoc_aniso_dev)": lambda: e.ekf_update_assoc_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, anc, n, COV, tabs["aniso"], Lp, None),
        "table update, Q_k (slam_ekf_update_assoc_detcov_dev)": lambda: e.ekf_update_assoc_detcov_dev(d_in, d_out, 5 * Lp, Lp, L, *pose, anc, n, tabs["detcov"], Lp, None),
    }, pkg.Engine.PROF_EKF)
e.close()
