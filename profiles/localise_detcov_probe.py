#!/usr/bin/env python3
"""profiles/localise_detcov_probe.py [N L ROUNDS REPS] — what localising in a known map under a covariance per detection costs
(slam_localise_detcov_dev) against the only way to do the same job without it: a rows population whose every particle holds a copy
of the map, slam_associate_detcov_dev(create = 0) plus slam_ekf_update_assoc_detcov_dev — and, as the floor, slam_localise_dev on
the prepared map under meas_var * I.  On the GPU, through the package, in ONE process.  Default 65 536 particles x 500 landmarks,
K = 16 detections with the range model's covariances; 6 rounds of 20 launches, the variants interleaved round by round, each launch
timed by the events around it (SLAM_PROF_PAGES for the stages and the association, SLAM_PROF_EKF for the update); one warm-up
round first.

The rows path needs 2 x 20 B per (particle, landmark) of device memory (source and destination rows) plus the table; it is timed
only if that allocates.  Per variant the median, minimum and maximum over the rounds, the bytes it moves by its own model and the
device memory it needs.  Measurement tooling: prints, asserts nothing about time (it does assert that both per-detection paths
agree on the stats and the log-likelihood's bits where both ran)."""
import statistics
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "6", "20"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, Q, GATE, K = "cuda:0", 0.01, 9.21, 16
RANGE_VAR, BEARING_VAR, LATERAL_VAR = 1e-4, 1.5625e-4, 1e-4
pkg = load_package()
rng = np.random.default_rng(1)
M = np.zeros((5, Lp), np.float32)
M[2] = -1.0
M[0, :L], M[1, :L] = rng.uniform(-50, 50, L), rng.uniform(-50, 50, L)
M[2, :L], M[4, :L] = 0.05, 0.05
true = np.array([3.0, -2.0, 0.5])
near = np.argsort(np.hypot(M[0, :L] - true[0], M[1, :L] - true[1]))[:K]
c, s = np.cos(true[2]), np.sin(true[2])
dx, dy = M[0, near] - true[0], M[1, near] - true[1]
zx, zy = c * dx - s * dy, s * dx + c * dy
r2 = zx * zx + zy * zy
ux, uy = zx / np.sqrt(r2), zy / np.sqrt(r2)
a, b = RANGE_VAR, BEARING_VAR * r2 + LATERAL_VAR
covs = tuple(v.astype(np.float32) for v in (a * ux * ux + b * uy * uy, (a - b) * ux * uy, a * uy * uy + b * ux * ux))
zx, zy = zx.astype(np.float32), zy.astype(np.float32)
x = (true[0] + 0.3 * rng.standard_normal(n)).astype(np.float32)
y = (true[1] + 0.3 * rng.standard_normal(n)).astype(np.float32)
th = (true[2] + 0.03 * rng.standard_normal(n)).astype(np.float32)


def report(name, t, moved, held):
    print(f"  {name:44s} median {statistics.median(t):9.1f} us   min {min(t):9.1f} us   max {max(t):9.1f} us   spread {max(t) - min(t):7.1f} us"
          f"   moves {moved / 1e6:10.2f} MB   holds {held / 1e9:8.3f} GB")


e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
e.detections_upload(zx, zy)
e.detections_cov_upload(*covs)
d_x, d_y, d_th = (torch.as_tensor(v).to(DEV) for v in (x, y, th))
d_M = torch.as_tensor(M).to(DEV)
d_prep = torch.empty((6, Lp), device=DEV)
d_st = torch.empty((n, 3), dtype=torch.int32, device=DEV)
d_ll = torch.empty((n,), device=DEV)
d_st0 = torch.empty((n, 3), dtype=torch.int32, device=DEV)
d_ll0 = torch.empty((n,), device=DEV)
e.known_map_prepare_dev(d_M, Lp, L, Q, d_prep)

rows = None
try:
    d_in = d_M.unsqueeze(0).expand(n, 5, Lp).contiguous()      # every particle its own copy of the map
    d_out = torch.empty_like(d_in)
    d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
    d_st2 = torch.empty((n, 3), dtype=torch.int32, device=DEV)
    d_ll2 = torch.empty((n,), device=DEV)
    torch.cuda.synchronize()
    rows = True
except RuntimeError as err:   # (out of device memory: the rows path cannot do this shape at all)
    print(f"rows path: does not allocate at {n} x {L} ({2 * n * 5 * Lp * 4 / 1e9:.1f} GB of rows): {str(err).splitlines()[0]}")
    d_in = d_out = d_assoc = None
    torch.cuda.empty_cache()


def timed(kernel, fn):
    e.profile_read(kernel)
    for _ in range(reps):
        fn()
    e.sync()
    ms, cnt = e.profile_read(kernel)
    assert cnt == reps
    return 1e3 * ms / cnt


stage = lambda: e.localise_detcov_dev(d_M, Lp, L, d_x, d_y, d_th, n, GATE, None, 0, d_st, d_ll)
floor = lambda: e.localise_dev(d_prep, Lp, L, d_x, d_y, d_th, n, GATE, None, 0, d_st0, d_ll0)
assoc = lambda: e.associate_detcov_dev(d_in, 5 * Lp, Lp, L, d_x, d_y, d_th, None, n, GATE, GATE, 0, d_assoc, Lp, d_st2)
update = lambda: e.ekf_update_assoc_detcov_dev(d_in, d_out, 5 * Lp, Lp, L, d_x, d_y, d_th, None, n, d_assoc, Lp, d_ll2)
e.profile_enable(e.PROF_PAGES, e.PROF_EKF)
t = {"stage": [], "floor": [], "assoc": [], "update": []}
for r in range(rounds + 1):   # (round 0: warm-up)
    got = dict(stage=timed(e.PROF_PAGES, stage), floor=timed(e.PROF_PAGES, floor))
    if rows:
        got.update(assoc=timed(e.PROF_PAGES, assoc), update=timed(e.PROF_EKF, update))
    if r:
        for k, v in got.items():
            t[k].append(v)
e.profile_enable()
print(f"n = {n}, L = {L} (plane stride {Lp}), K = {K}; {rounds} rounds of {reps} launches; matched per particle: "
      f"{d_st[:, 0].float().mean().item():.2f} (per detection), {d_st0[:, 0].float().mean().item():.2f} (isotropic, meas_var {Q})")
report("slam_localise_detcov_dev (no table)", t["stage"], n * (12 + 16) + 5 * Lp * 4, 5 * Lp * 4 + n * (12 + 12 + 4))
report("slam_localise_dev (no table; the floor)", t["floor"], n * (12 + 16) + 6 * Lp * 4, 6 * Lp * 4 + n * (12 + 12 + 4))
if rows:
    held_rows = 2 * n * 5 * Lp * 4 + n * Lp + n * (12 + 12 + 4)
    report("slam_associate_detcov_dev(create = 0)", t["assoc"], n * (5 * Lp * 4 + Lp + 12 + 12), held_rows)
    report("slam_ekf_update_assoc_detcov_dev", t["update"], n * (2 * 5 * Lp * 4 + Lp + 12 + 4), held_rows)
    report("  the two together", [p + q for p, q in zip(t["assoc"], t["update"])], n * (3 * 5 * Lp * 4 + 2 * Lp + 40), held_rows)
    torch.cuda.synchronize()
    assert torch.equal(d_st, d_st2) and torch.equal(d_ll.view(torch.int32), d_ll2.view(torch.int32)), "the two paths disagree"
    print("  stats and log-likelihood bits of the two per-detection paths are equal")
e.close()
