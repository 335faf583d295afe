#!/usr/bin/env python3
"""profiles/assoc_weight_measure.py [N L ROUNDS REPS] — what weighing the unexplained costs (slam_assoc_weight_dev, the miss count
of the evidence stage, slam_pf_assoc_weight_set) on the GPU, through the package, in ONE process.  Default: 65 536 particles x 64
slots (plane stride 64), K = 16 detections, pruning on; 6 rounds of 20 launches.

Stage by stage, interleaved round by round and each timed by the events around its own launch (SLAM_PROF_PAGES):
  * the evidence stage, plain and with field of view + line of sight, WITHOUT the miss count (a null pointer: the call a tree
    without the feature has too) and WITH it, out of place behind ancestors on the rows an associating update wrote;
  * slam_assoc_weight_dev on the engine's log-likelihood buffer.
Then a rows session of the same shape, frame by frame (wall clock, one synchronisation per frame): the switch never given, and the
switch on.
Run from a checkout that lacks the feature, the script measures what that checkout has — the evidence stage without the count and
the frame without the switch — which is how the parent commit's figures in profiles/assoc_weight.md were made: the same script,
copied into a checkout of the parent.
Per variant the median, minimum and maximum over the rounds; the SPREAD of a variant is max - min.  Measurement tooling: prints,
asserts nothing about time."""
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
import _shard_worker as W  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "64", "6", "20"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, Q, GATE, NEW_GATE, K = "cuda:0", 2.5e-3, 9.21, 50.0, 16
HIT, MISS, CMAX, RANGE, MARGIN = 1, 1, 8, 9.0, 0.3
CONSTS = (-4.0, -1.5, -0.75)
pkg = load_package()
HAS = hasattr(pkg.Engine, "assoc_weight_dev")
meta, edt, bx, by, lm = W.make_world(L=L)
x, y, th, mp = W.init_state(n, L, lm)
mp[:, 2, L // 2:] = -1.0                                  # half of the slots free: detections beyond them start landmarks
rng = np.random.default_rng(1)
z = np.concatenate([lm[:K // 2], rng.uniform(-3, 3, (K - K // 2, 2)).astype(np.float32)])   # half on landmarks, half anywhere


def report(name, t):
    print(f"  {name:62s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   spread {max(t) - min(t):6.1f} us")


def stages():
    e = pkg.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.scan_upload(bx, by)
    e.detections_upload(z[:, 0].copy(), z[:, 1].copy())
    e.sight_table_dev(128)
    d_x, d_y, d_th = (torch.as_tensor(v).to(DEV) for v in (x, y, th))
    heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
    anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
    d_in = torch.zeros((n, 5, Lp), device=DEV)
    d_in[:, :, :L] = torch.as_tensor(mp).to(DEV)
    d_out = torch.empty_like(d_in)
    d_work = torch.empty_like(d_in)
    d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
    d_astats = torch.empty((n, 3), dtype=torch.int32, device=DEV)
    e.associate_dev(d_in, 5 * Lp, Lp, L, d_x, d_y, d_th, anc, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, d_astats)
    e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, d_x, d_y, d_th, anc, n, Q, d_assoc, Lp, None)
    d_ev_in = torch.full((n, Lp), 3, dtype=torch.uint8, device=DEV)
    d_ev_out = torch.empty_like(d_ev_in)
    d_st = torch.empty((n, 2), dtype=torch.int32, device=DEV)
    d_sp, d_ou, d_ms = (torch.empty((n,), dtype=torch.int32, device=DEV) for _ in range(3))
    lo, hi = float(pkg.fov_bound(-2.351831 + 0.1)), float(pkg.fov_bound(2.351831 - 0.1))
    head = (d_work, 5 * Lp, Lp, L, d_x, d_y)
    mid = (anc, n, d_assoc, Lp, d_ev_in, d_ev_out, Lp, HIT, MISS, CMAX, RANGE)
    variants = {"evidence, plain, without the miss count": lambda: e.landmark_evidence_dev(*head, *mid, d_st),
                "evidence, fov + sight, without the miss count": lambda: e.landmark_evidence_fov_dev(*head, d_th, *mid, MARGIN, lo, hi, True, d_st, d_sp, d_ou)}
    if HAS:
        variants["evidence, plain, with the miss count"] = lambda: e.landmark_evidence_dev(*head, *mid, d_st, d_missed=d_ms)
        variants["evidence, fov + sight, with the miss count"] = lambda: e.landmark_evidence_fov_dev(*head, d_th, *mid, MARGIN, lo, hi, True, d_st,
                                                                                                      d_sp, d_ou, d_missed=d_ms)
        variants["slam_assoc_weight_dev (engine's buffer, with missed)"] = lambda: e.assoc_weight_dev(d_astats, d_ms, n, *CONSTS, None, None)
    for v in variants.values():
        d_work.copy_(d_out)
        v()
    e.sync()
    a = d_astats.sum(dim=0).cpu().numpy() / n
    print(f"{n} x {L} (plane stride {Lp}), K = {K}; per particle matched {a[0]:.2f} created {a[1]:.2f} dropped {a[2]:.2f}"
          + (f" missed {d_ms.sum().item() / n:.2f}" if HAS else "") + f"; {rounds} rounds x {reps} launches")
    times = {v: [] for v in variants}
    for _ in range(rounds):
        for name, v in variants.items():
            d_work.copy_(d_out)                             # the rows the update wrote (a prune writes into them)
            e.sync()
            e.profile_enable(pkg.Engine.PROF_PAGES)
            for _ in range(reps):
                v()
            e.sync()
            ms, launches = e.profile_read(pkg.Engine.PROF_PAGES)
            assert launches == reps
            times[name].append(1e3 * ms / launches)
            e.profile_enable()
    for name, t in times.items():
        report(name, t)
    e.close()


def session_frames(on, frames=30):
    e = pkg.Engine(0)
    d_edt = torch.from_numpy(edt).to(DEV)
    e.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    e.scan_upload(bx, by)
    ses = pkg.PfSession(e, n, L, map_layout="rows", seed=5, sigma=(0.005, 0.005, 0.001), meas_var=Q, score_gain=0.05)
    ses.assoc_set(GATE, NEW_GATE, True)
    ses.set_poses(x, y, th)
    ses.set_map(mp)
    ses.prune_set(HIT, MISS, CMAX, RANGE)
    if on:
        ses.assoc_weight_set(*CONSTS)
    t = []
    for f in range(frames):
        e.detections_upload(z[:, 0].copy(), z[:, 1].copy())
        e.sync()
        t0 = time.perf_counter()
        ses.step(0, [0.0, 0.0, 0.0], True)
        e.sync()
        t.append(1e6 * (time.perf_counter() - t0))
    ses.close()
    e.close()
    return statistics.median(t[5:])


stages()
sys.stdout.flush()
SROUNDS = 5
print(f"session frame, {n} x {L} rows, association + pruning, K = {K} uploaded detections; median of frames 5 .. 29, {SROUNDS} rounds:")
names = {"the switch never given": False}
if HAS:
    names["the switch on"] = True
frames = {k: [] for k in names}
for _ in range(SROUNDS):
    for name, on in names.items():
        frames[name].append(session_frames(on))
for name, t in frames.items():
    report(name, t)
