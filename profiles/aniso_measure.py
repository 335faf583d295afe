#!/usr/bin/env python3
"""profiles/aniso_measure.py [N L ROUNDS REPS] — SLAM_PROF_EKF of the landmark update with a 2x2 measurement covariance
(slam_ekf_update_aniso_dev) beside the isotropic one-wavefront-per-particle kernel (slam_ekf_update_dev under
slam_ekf_form_set(e, 0)), in ONE process on the same inputs: out of place through resampled ancestors, every landmark
observed.  The two are alternated in blocks of REPS launches for ROUNDS rounds (after a warm-up of each); per kernel the
median and the minimum over the rounds of the mean launch time, and the ratio of the medians.  Measurement tooling: prints,
asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), 12 rounds of 20 launches."""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "12", "20"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV = "cuda:0"
pkg = load_package()
e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
x, y, th = (torch.as_tensor(rng.uniform(-5, 5, n).astype(np.float32)).to(DEV) for _ in range(3))
# resampled ancestors: ~6 % distinct, the offspring of one ancestor neighbours (what a systematic resample leaves)
heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
rows = rng.uniform(-10, 10, (n, 5, Lp)).astype(np.float32)
rows[:, 2], rows[:, 3], rows[:, 4] = 0.05, 0.01, 0.04
d_in, d_out = torch.as_tensor(rows).to(DEV), torch.empty((n, 5, Lp), device=DEV)
z = rng.uniform(-10, 10, (2, L)).astype(np.float32)
e.obs_upload(np.arange(L, dtype=np.int32), z[0], z[1], L)
e.ekf_form_set(0)
cov = (0.02, 0.012, 0.015)
calls = {
    "isotropic, form 0 (ekf_update_kernel)": lambda: e.ekf_update_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, 0.02, None),
    "2x2 Q (ekf_update_kernel, EkfNoiseAniso)": lambda: e.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, cov, None),
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
print(f"{n} x {L} (plane stride {Lp}), every landmark observed, {len(heads)} distinct ancestors; {rounds} rounds x {reps} launches, alternating")
med = {}
for name, t in times.items():
    med[name] = statistics.median(t)
    print(f"  {name:40s} median {med[name]:8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us")
a, b = (med[k] for k in calls)
print(f"  ratio 2x2 Q / isotropic (medians): {b / a:.3f}")
e.close()
