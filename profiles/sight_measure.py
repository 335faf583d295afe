#!/usr/bin/env python3
"""profiles/sight_measure.py [N L ROUNDS REPS] — the existence-evidence stage with line of sight on the GPU, through the package, in
ONE process, on the scene and the shape of profiles/evidence_measure.py:
  * slam_landmark_evidence_dev (SLAM_PROF_PAGES) behind slam_ekf_update_assoc_dev on the rows that launch wrote — the stage as it is,
  * slam_landmark_evidence_sight_dev (SLAM_PROF_PAGES) behind the same update on the same rows, through the same ancestors, table and
    evidence, reading the sight table (128 bins, margin 0.3) of a 360-beam scan whose returns lie 8 .. 20 m out, so that some of
    the landmarks due a miss are hidden and some are not,
  * slam_sight_table_dev (SLAM_PROF_PAGES) by itself.
Rounds of the two stages alternate (REPS pairs of update + stage each), ROUNDS rounds per stage after a warm-up; per kernel the
median, minimum and maximum over the rounds of the mean launch time, and the ratio of the medians.  Measurement tooling: prints,
asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), 6 rounds of 10 pairs."""
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
HIT, MISS, CMAX, RANGE = 1, 1, 8, 15.0
BINS, MARGIN, NBEAMS = 128, 0.3, 360
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
d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_ev_in = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_ev_out = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_stats = torch.empty((n, 2), dtype=torch.int32, device=DEV)
d_spared = torch.empty((n,), dtype=torch.int32, device=DEV)
K = min(56, L)
ids = rng.permutation(L)[:K]
zx = np.concatenate([lm[ids, 0], rng.uniform(-20, 20, 8).astype(np.float32)])   # (the pose is the origin, heading 0: z = m)
zy = np.concatenate([lm[ids, 1], rng.uniform(-20, 20, 8).astype(np.float32)])
e.detections_upload(zx, zy)
ang = -np.pi + 2 * np.pi * np.arange(NBEAMS) / NBEAMS
rad = rng.uniform(8.0, 20.0, NBEAMS)
e.scan_upload((rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32))
e.sight_table_dev(BINS)
e.associate_dev(d_in, 5 * Lp, Lp, L, x, y, th, anc, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, None)
e.evidence_init_dev(d_in, 5 * Lp, Lp, L, n, d_ev_in, Lp, 3)
d_ev_in = torch.minimum(d_ev_in, torch.randint(0, 4, (n, Lp), dtype=torch.uint8, device=DEV))


def pair(sight):
    e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, Q, d_assoc, Lp, None)
    if sight:
        e.landmark_evidence_sight_dev(d_out, 5 * Lp, Lp, L, x, y, th, anc, n, d_assoc, Lp, d_ev_in, d_ev_out, Lp, HIT, MISS, CMAX, RANGE,
                                      MARGIN, d_stats, d_spared)
    else:
        e.landmark_evidence_dev(d_out, 5 * Lp, Lp, L, x, y, anc, n, d_assoc, Lp, d_ev_in, d_ev_out, Lp, HIT, MISS, CMAX, RANGE, d_stats)


def report(name, t):
    print(f"  {name:58s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us")
    return statistics.median(t)


print(f"{n} x {L} (plane stride {Lp}), {len(heads)} distinct ancestors, K = {len(zx)}, {NBEAMS} beams, {BINS} bins; {rounds} rounds x {reps} pairs")
for sight in (False, True):
    for _ in range(5):
        pair(sight)
    e.sync()
    st = d_stats.sum(dim=0).cpu().numpy() / n
    print(f"      {'with' if sight else 'without'} sight, per particle: pruned {st[0]:.2f}  seen after pruning {st[1]:.2f}"
          + (f"  spared {d_spared.sum().item() / n:.2f}" if sight else ""))
e.profile_enable(pkg.Engine.PROF_EKF, pkg.Engine.PROF_PAGES)
times = {"slam_landmark_evidence_dev": [], "slam_landmark_evidence_sight_dev": []}
update = []
for _ in range(rounds):
    for sight, name in zip((False, True), times):
        for _ in range(reps):
            pair(sight)
        e.sync()
        ms, launches = e.profile_read(pkg.Engine.PROF_PAGES)
        assert launches == reps
        times[name].append(1e3 * ms / launches)
        ms, launches = e.profile_read(pkg.Engine.PROF_EKF)
        update.append(1e3 * ms / launches)
u = report("slam_ekf_update_assoc_dev in front of either", update)
a, b = (report(name, t) for name, t in times.items())
table = []
for _ in range(rounds):
    for _ in range(reps):
        e.sight_table_dev(BINS)
    e.sync()
    ms, launches = e.profile_read(pkg.Engine.PROF_PAGES)
    assert launches == reps
    table.append(1e3 * ms / launches)
report("slam_sight_table_dev", table)
print(f"  ratio sight stage / stage (medians): {b / a:.3f}; sight stage / assoc update: {b / u:.3f}")
e.profile_enable()
e.close()
