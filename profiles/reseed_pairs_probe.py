#!/usr/bin/env python3
"""profiles/reseed_pairs_probe.py [ROUNDS REPS] — what slam_pf_known_map_reseed_pairs costs beside the frame it follows and beside
slam_pf_known_map_reseed.  On the GPU, through the package, in ONE process: sessions of 65 536 and 1 048 576 particles in known
maps of 50 and 500 landmarks (uniform over 50 m x 50 m) with 12 detections — twelve of the map's landmarks seen from one pose —
fraction 1/16 and 1, tol 0.07 m, min_sep 1.5 m.  Default 6 rounds of 20 calls, the variants interleaved round by round, one warm-up
round first.  Every call blocks the host until its counts are there, so each is timed twice: by HIP events on the engine's stream
around the calls (the device's share) and by the host's clock (what the caller waits).

Measurement tooling: prints, asserts nothing about time (it does assert that the counts add up to what the fraction chooses,
within 5 sigma of the binomial, and that some proposals are made)."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

rounds, reps = (int(v) for v in (sys.argv[1:3] + ["6", "20"][len(sys.argv) - 1:]))
pkg = load_package()
rng = np.random.default_rng(7)
rows, cols, ld = 150, 190, 200
occ = np.zeros((ld, ld), np.int32)
occ[:rows, :cols] = rng.random((rows, cols)) < 0.02
ang = np.linspace(-np.pi, np.pi, 360, endpoint=False)
rad = rng.uniform(1.0, 6.0, 360)
bx, by = (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)
K, TOL, MIN_SEP = 12, 0.07, 1.5


def world(L):
    """-> (M [5][L], zx, zy): the K landmarks nearest to a pose, seen from it exactly (z = H(theta) (m - p))."""
    r = np.random.default_rng(100 + L)
    M = np.zeros((5, L), np.float32)
    M[0], M[1] = r.uniform(-25, 25, (2, L))
    M[2] = M[4] = 0.05
    px, py, t = 3.0, -2.0, 0.6
    dx, dy = M[0].astype(np.float64) - px, M[1].astype(np.float64) - py
    near = np.argsort(np.hypot(dx, dy))[:K]
    zx, zy = np.cos(t) * dx[near] - np.sin(t) * dy[near], np.sin(t) * dx[near] + np.cos(t) * dy[near]
    return M, zx.astype(np.float32), zy.astype(np.float32)


def report(name, dev, wall):
    for what, t in (("device", dev), ("host  ", wall)):
        print(f"  {name:52s} {what} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   "
              f"spread {max(t) - min(t):7.1f} us")


def timed(fn):
    """reps calls -> (device us per call between two events on the engine's stream, host us per call)"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps, 1e6 * (time.perf_counter() - t0) / reps


for n in (65536, 1048576):
    for L in (50, 500):
        M, zx, zy = world(L)
        e = pkg.Engine(0)
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.grid_upload(0, occ, pkg.grid_meta(rows, cols, ld, 0.1, -3.0, -2.5), 10.0)
        e.scan_upload(bx, by)
        ses = pkg.PfSession(e, n, 0, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.25, seed=3)
        ses.set_poses((6.0 + 0.3 * rng.standard_normal(n)).astype(np.float32), (5.0 + 0.3 * rng.standard_normal(n)).astype(np.float32),
                      (0.1 * rng.standard_normal(n)).astype(np.float32))
        ses.known_map_set(M, 9.21, -2.5)
        e.detections_upload(zx, zy)

        def frame_then(fn):
            """a step first, so that every call finds what it finds in use: a pending resample to apply"""
            ses.step(0, [0.01, -0.005, 0.002], True)
            return fn()

        shares = {}
        for fraction in (1.0 / 16, 1.0):
            got = frame_then(lambda: ses.known_map_reseed_pairs(fraction, TOL, MIN_SEP))
            sigma = (n * fraction * (1 - fraction)) ** 0.5
            assert abs(sum(got) - n * fraction) <= 5 * sigma + 0.5 and got[0] > 0 and got[1] == 0, got
            shares[fraction] = got
        variants = {"step": lambda: e.sync(),
                    "single 1/16": lambda: ses.known_map_reseed(1.0 / 16),
                    "single 1": lambda: ses.known_map_reseed(1.0),
                    "pairs 1/16": lambda: ses.known_map_reseed_pairs(1.0 / 16, TOL, MIN_SEP),
                    "pairs 1": lambda: ses.known_map_reseed_pairs(1.0, TOL, MIN_SEP)}
        t = {k: ([], []) for k in variants}
        for rd in range(rounds + 1):   # (round 0: warm-up)
            for k, fn in variants.items():
                dv, hv = timed(lambda fn=fn: frame_then(fn))
                if rd:
                    t[k][0].append(dv)
                    t[k][1].append(hv)
        print(f"n = {n}, {L} landmarks, {K} detections; {rounds} rounds of {reps} calls, each behind one slam_pf_step (use_observations = 1)")
        for fraction, got in shares.items():
            print(f"  fraction {fraction:.4f}: replaced {got[0]}, j1 empty {got[1]}, too close {got[2]}, no partner {got[3]}")
        report("slam_pf_step + sync (the frame alone)", *t["step"])
        report("... + slam_pf_known_map_reseed(1/16)", *t["single 1/16"])
        report("... + slam_pf_known_map_reseed(1)", *t["single 1"])
        report("... + slam_pf_known_map_reseed_pairs(1/16)", *t["pairs 1/16"])
        report("... + slam_pf_known_map_reseed_pairs(1)", *t["pairs 1"])
        base = statistics.median(t["step"][1])
        for k in list(variants)[1:]:
            print(f"  host time beyond the frame, {k}: {statistics.median(t[k][1]) - base:9.1f} us")
        ses.close()
        e.close()
