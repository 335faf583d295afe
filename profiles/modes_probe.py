#!/usr/bin/env python3
"""profiles/modes_probe.py [ROUNDS REPS] — what slam_pf_modes costs against slam_pf_spread ("one more pass over 12 B per particle")
and against the only way to have the modes without it: slam_pf_get_poses_host plus NumPy on the host.  On the GPU, through the
package, in ONE process: sessions of 65 536 and 1 048 576 particles on three clouds — settled (sigma = 1 cm), two clusters, a
uniform scatter over 50 m x 50 m — with cell = 0.5 m and 16 heading bins.  Default 6 rounds of 20 calls, the variants interleaved
round by round, one warm-up round first.  Every call blocks the host until its result is there, so each is timed twice: by HIP
events on the engine's stream around the calls (the device's share) and by the host's clock (what the caller waits).

A/B of the accumulate kernel's shape: build the library a second time with the wave-level and LDS combining compiled out,
    make -C hardware-acceleration-of-lidar-slam_amd/csrc OUT=../lib_modes_nocombine EXTRA=-DSLAM_MODES_NO_COMBINE
and run this probe again with SLAM_HIP_LIB=<package>/lib_modes_nocombine/libslam_hip.so: the "slam_pf_modes" lines of that run are the
same three launches with one set of memory atomics per particle (two processes: compare medians, not single rounds).

Measurement tooling: prints, asserts nothing about time (it does assert that the heaviest mode of the host restatement is the
call's)."""
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
CELL, HB, MM = 0.5, 16, 4
print(f"library: {pkg.LIB_PATH}")


def clouds(n, rng):
    yield "settled", (rng.normal(6.1, 0.01, n), rng.normal(5.2, 0.01, n), rng.normal(0.1, 0.01, n))
    side = np.arange(n) % 2
    yield "two clusters", (np.where(side, 4.0, -4.0) + rng.normal(0, 0.01, n), rng.normal(1.0, 0.01, n),
                           np.where(side, 0.5 + np.pi, 0.5) + rng.normal(0, 0.01, n))
    yield "scatter 50 m", (rng.uniform(-25, 25, n), rng.uniform(-25, 25, n), rng.uniform(-np.pi, np.pi, n))


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return 1e3 * a.elapsed_time(b) / reps, 1e6 * (time.perf_counter() - t0) / reps


def host_modes(ses):
    """copy-out and a NumPy restatement of the heaviest mode (float64 cells, no exactness): what an application does today"""
    x, y, th = ses.poses()
    ix, iy = np.floor(x / CELL).astype(np.int64), np.floor(y / CELL).astype(np.int64)
    b = np.minimum(((th / (2 * np.pi)) % 1.0 * HB).astype(np.int64), HB - 1)
    keys, counts = np.unique((ix + (1 << 20)) << 27 | (iy + (1 << 20)) << 6 | b, return_counts=True)
    table = dict(zip(keys.tolist(), counts.tolist()))
    best = (0, None)
    for k in keys.tolist():
        kx, ky, kb = k >> 27, (k >> 6) & 0x1fffff, k & 63
        sc = sum(table.get((kx + dx) << 27 | (ky + dy) << 6 | (kb + db) % HB, 0) for dx in (-1, 0, 1) for dy in (-1, 0, 1) for db in (-1, 0, 1))
        if sc > best[0]:
            best = (sc, (kx - (1 << 20), ky - (1 << 20), kb))
    return best


def report(name, dev, wall, moved):
    for what, t in (("device", dev), ("host  ", wall)):
        print(f"  {name:34s} {what} median {statistics.median(t):9.1f} us   min {min(t):9.1f} us   max {max(t):9.1f} us"
              + (f"   moves {moved / 1e6:8.2f} MB" if what == "device" else ""))


for n in (65536, 1048576):
    rng = np.random.default_rng(7)
    e = pkg.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    ses = pkg.PfSession(e, n, 0, sigma=(0.02, 0.02, 0.004), seed=3)
    for name, pop in clouds(n, rng):
        ses.set_poses(*(np.asarray(a, np.float32) for a in pop))
        def ask():
            try:
                return ses.modes(0.1, CELL, HB, MM)
            except pkg.SlamError as exc:      # (the scatter at 1 048 576 particles fills all 160 000 cells: SLAM_ERR_CAPACITY, still timed)
                return [], str(exc)

        modes, cells = ask()
        variants = {"spread": lambda: ses.spread(0.1), "modes": ask}
        if name != "scatter 50 m":              # (the restatement's Python loop over tens of thousands of cells takes seconds: not timed)
            score, centre = host_modes(ses)
            assert modes[0]["weight"] == score and modes[0]["cell"] == centre, (modes[0], score, centre)
            variants["copy"] = lambda: host_modes(ses)
        t = {k: ([], []) for k in variants}
        for rd in range(rounds + 1):   # (round 0: warm-up)
            got = {k: timed(fn) for k, fn in variants.items()}
            if rd:
                for k, (dv, hv) in got.items():
                    t[k][0].append(dv)
                    t[k][1].append(hv)
        print(f"n = {n}, {name}: {cells} cells, {len(modes)} modes, masses {[round(float(m['mass']), 4) for m in modes]}; "
              f"{rounds} rounds of {reps} calls")
        report("slam_pf_spread", *t["spread"], 24 * n)
        report("slam_pf_modes", *t["modes"], 12 * n)
        if "copy" in t:
            report("slam_pf_get_poses_host + NumPy", *t["copy"], 12 * n)
    ses.close()
    e.close()
