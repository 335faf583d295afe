#!/usr/bin/env python3
"""profiles/reseed_probe.py [ROUNDS REPS] — what slam_pf_known_map_reseed costs against the round trip it replaces:
slam_pf_get_poses_host followed by slam_pf_set_poses_host (the host's own invention of poses in between is NOT counted: the round
trip alone).  On the GPU, through the package, in ONE process: sessions of 65 536 and 1 048 576 particles in a known map of 50
landmarks with 12 detections, fraction 1/16 and 1.  Default 6 rounds of 20 calls, the variants interleaved round by round, one
warm-up round first.  Every call blocks the host until its result is there, so each is timed twice: by HIP events on the engine's
stream around the calls (the device's share) and by the host's clock (what the caller waits).

Measurement tooling: prints, asserts nothing about time (it does assert that the counts add up to what the fraction chooses,
within 5 sigma of the binomial)."""
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
L, K = 50, 12
M = np.zeros((5, L), np.float32)
M[0], M[1] = rng.uniform(-25, 25, (2, L))
M[2] = M[4] = 0.05
zx, zy = rng.uniform(-8, 8, (2, K)).astype(np.float32)


def report(name, dev, wall, moved):
    for what, t in (("device", dev), ("host  ", wall)):
        print(f"  {name:44s} {what} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   "
              f"spread {max(t) - min(t):7.1f} us" + (f"   moves {moved / 1e6:8.2f} MB" if what == "device" else ""))


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

    def round_trip():
        p = ses.poses()
        ses.set_poses(p[0], p[1], p[2])

    for fraction in (1.0 / 16, 1.0):
        got = frame_then(lambda: ses.known_map_reseed(fraction))
        sigma = (n * fraction * (1 - fraction)) ** 0.5
        assert abs(sum(got) - n * fraction) <= 5 * sigma + 0.5 and got[1] == 0, got
    t = {k: ([], []) for k in ("step", "reseed 1/16", "reseed 1", "round trip")}
    for rd in range(rounds + 1):   # (round 0: warm-up)
        got = {"step": timed(lambda: frame_then(lambda: e.sync())),
               "reseed 1/16": timed(lambda: frame_then(lambda: ses.known_map_reseed(1.0 / 16))),
               "reseed 1": timed(lambda: frame_then(lambda: ses.known_map_reseed(1.0))),
               "round trip": timed(lambda: frame_then(round_trip))}
        if rd:
            for k, (dv, hv) in got.items():
                t[k][0].append(dv)
                t[k][1].append(hv)
    print(f"n = {n}, {L} landmarks, {K} detections; {rounds} rounds of {reps} calls, each behind one slam_pf_step (use_observations = 1)")
    report("slam_pf_step + sync (the frame alone)", *t["step"], 0)
    report("... + slam_pf_known_map_reseed(1/16)", *t["reseed 1/16"], 28 * n)
    report("... + slam_pf_known_map_reseed(1)", *t["reseed 1"], 12 * n)
    report("... + get_poses_host + set_poses_host", *t["round trip"], 24 * n)
    base = statistics.median(t["step"][1])
    for k in ("reseed 1/16", "reseed 1", "round trip"):
        print(f"  host time beyond the frame, {k}: {statistics.median(t[k][1]) - base:9.1f} us")
    ses.close()
    e.close()
