#!/usr/bin/env python3
"""profiles/spread_probe.py [ROUNDS REPS] — what slam_pf_spread costs against slam_pf_mean and against the only way to have a
covariance without it: slam_pf_get_poses_host plus NumPy on the host.  On the GPU, through the package, in ONE process: sessions of
65 536 and 1 048 576 particles, resampling every frame ("plain") and ESS-gated on a frame the gate kept ("gated": the weighted
forms).  Default 6 rounds of 20 calls, the three variants interleaved round by round, one warm-up round first.  Every call blocks
the host until its result is there, so each is timed twice: by HIP events on the engine's stream around the call (the device's
share) and by the host's clock (what the caller waits).

Per variant the median, minimum, maximum and spread over the rounds and the bytes it moves by its own model.  Measurement tooling:
prints, asserts nothing about time (it does assert that the pose of spread is the mean's, bit for bit, and that the covariance
agrees with NumPy's to float32 accuracy on plain frames)."""
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


def report(name, dev, wall, moved):
    for what, t in (("device", dev), ("host  ", wall)):
        print(f"  {name:34s} {what} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   "
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


def host_cov(ses):
    p = ses.poses().astype(np.float64)
    m = p.mean(axis=1)
    d = np.stack([p[0] - m[0], p[1] - m[1], np.sin(p[2] - m[2])])
    return (d @ d.T) / p.shape[1]


for n in (65536, 1048576):
    for gated in (False, True):
        e = pkg.Engine(0)
        e.set_stream(torch.cuda.current_stream().cuda_stream)
        e.grid_upload(0, occ, pkg.grid_meta(rows, cols, ld, 0.1, -3.0, -2.5), 10.0)
        e.scan_upload(bx, by)
        ses = pkg.PfSession(e, n, 0, sigma=(0.02, 0.02, 0.004), score_gain=0.002 if gated else 0.25, seed=3,
                            resample_ess_frac=0.5 if gated else 0.0)
        ses.set_poses((6.0 + 0.3 * rng.standard_normal(n)).astype(np.float32), (5.0 + 0.3 * rng.standard_normal(n)).astype(np.float32),
                      (0.1 * rng.standard_normal(n)).astype(np.float32))
        for _ in range(3):
            ses.step(0, [0.01, -0.005, 0.002])
        kept = gated and not e.resample_happened()
        if kept != gated:
            print("  (the gated session's last frame was NOT one the gate kept: the figures below are the plain forms)")
        pose, cov, r = ses.spread(0.1)
        assert np.array_equal(pose.view(np.uint32), ses.mean(0.1).view(np.uint32))
        if not gated:
            c = host_cov(ses)
            want = np.array([c[0, 0], c[0, 1], c[1, 1], c[0, 2], c[1, 2], c[2, 2]])
            assert np.allclose(cov, want, rtol=1e-3, atol=1e-6), (cov, want)
        t = {k: ([], []) for k in ("mean", "spread", "copy")}
        for rd in range(rounds + 1):   # (round 0: warm-up)
            got = {"mean": timed(lambda: ses.mean(0.1)), "spread": timed(lambda: ses.spread(0.1)), "copy": timed(lambda: host_cov(ses))}
            if rd:
                for k, (dv, hv) in got.items():
                    t[k][0].append(dv)
                    t[k][1].append(hv)
        wbytes = 2 * n if gated else 0     # (the kernels read the carried log-weight, 4 B; the model counts the 16-bit weight it stands for)
        print(f"n = {n}, {'gated, the last frame kept (weighted forms)' if gated else 'plain'}; {rounds} rounds of {reps} calls; "
              f"sqrt(cov_xx + cov_yy) = {float(np.sqrt(cov[0] + cov[2])):.4f} m, heading_r = {float(r):.6f}")
        report("slam_pf_mean", *t["mean"], 12 * n + wbytes)
        report("slam_pf_spread", *t["spread"], 2 * (12 * n + wbytes))
        report("slam_pf_get_poses_host + NumPy", *t["copy"], 12 * n)
        ms, mc = statistics.median(t["spread"][1]), statistics.median(t["copy"][1])
        print(f"  host time, copy-out and NumPy / slam_pf_spread: {mc / ms:.1f} x;   slam_pf_spread / slam_pf_mean: "
              f"{ms / statistics.median(t['mean'][1]):.2f} x")
        ses.close()
        e.close()
