"""Measurement behind profiles/refine.md: slam_refine_poses_dev (one sweep) against what a user has without it — slam_score_poses_dev
on the explicit 27 n candidate poses, laid out beforehand pose-major (the 27 candidates of a pose side by side: the layout that
is kindest to the scorer's gathers; its arg-min is not counted) — and the frame time of a session with and without refinement.

One MI355X, one process, bench.py's synthetic room and scan, after the 250 ms settle bench.py uses; HIP-event medians.

    python profiles/refine_bench.py [--reps 60]      -> one JSON line per measurement
"""
import argparse
import json
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

STEPS = (0.025, 0.004363)   # the reference's fastResolution2


def median_us(torch, fn, reps):
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1e3


def world(torch, pkg, eng, grid, beams, landmarks=0, steps=8):
    args = SimpleNamespace(mode="pf" if landmarks else "score", landmarks=landmarks, grid=grid, beams=beams, steps=steps, warmup=0,
                           observed=0, preroll=0)
    inp = bench.build_inputs(args)
    dev = torch.device("cuda", 0)
    d_edt = torch.empty((grid, grid), dtype=torch.float32, device=dev)
    eng.edt_dev(torch.from_numpy(inp["occ"]).to(dev), grid, grid, grid, 10.0, d_edt)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(grid, grid, grid, inp["pixel"], inp["min_x"], inp["min_y"]))
    return inp, d_edt


def lattice_bench(torch, pkg, n, grid, beams, reps):
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    inp, keep = world(torch, pkg, eng, grid, beams)
    fr = inp["frames"][0]
    eng.scan_upload(fr["bx"], fr["by"])
    rng = np.random.default_rng(99)
    p0 = bench.true_pose(0)
    x = (p0[0] + rng.normal(0, 0.05, n)).astype(np.float32)
    y = (p0[1] + rng.normal(0, 0.05, n)).astype(np.float32)
    th = (p0[2] + rng.normal(0, 0.01, n)).astype(np.float32)
    t, r = np.float32(STEPS[0]), np.float32(STEPS[1])
    cand = np.empty((3, n, 27), np.float32)   # pose-major
    k = 0
    for a in (th - r, th, th + r):
        for xi in (x - t, x, x + t):
            for yj in (y - t, y, y + t):
                cand[0, :, k], cand[1, :, k], cand[2, :, k] = xi, yj, a
                k += 1
    d_c = torch.from_numpy(cand.reshape(3, -1)).to(dev)
    d_p0 = torch.from_numpy(np.stack([x, y, th])).to(dev)
    d_p = d_p0.clone()
    s27 = torch.empty(27 * n, device=dev)
    c27 = torch.empty(27 * n, device=dev, dtype=torch.int32)
    s, c = torch.empty(n, device=dev), torch.empty(n, device=dev, dtype=torch.int32)

    def refine():
        d_p.copy_(d_p0)   # the launch works in place: start from the same poses every time (the copy is timed alone and subtracted)
        eng.refine_poses_dev(0, d_p[0], d_p[1], d_p[2], n, STEPS[0], STEPS[1], 1, s, c)

    def restore_only():
        d_p.copy_(d_p0)

    def explicit():
        eng.score_poses_dev(0, d_c[0], d_c[1], d_c[2], 27 * n, s27, c27)

    bench.settle(torch)
    t_restore = median_us(torch, restore_only, reps)
    t_refine = median_us(torch, refine, reps) - t_restore
    t_explicit = median_us(torch, explicit, reps)
    # the two agree: the refined score is the incumbent-rule minimum of the explicit 27
    torch.cuda.synchronize()
    sc = s27.view(n, 27)
    best = sc[:, 13].clone()
    for k in range(27):
        best = torch.where(sc[:, k] < best, sc[:, k], best)
    refine()
    torch.cuda.synchronize()
    same = bool(torch.equal(best.view(torch.int32), s.view(torch.int32)))
    eng.close()
    return dict(what="lattice", poses=n, beams=beams, grid=grid, refine_us=round(t_refine, 1), explicit_27n_us=round(t_explicit, 1),
                ratio=round(t_explicit / t_refine, 2), restore_copy_us=round(t_restore, 1), scores_agree=same, reps=reps)


def session_bench(torch, pkg, n, L, grid, beams, sweeps, frames=40):
    dev = torch.device("cuda", 0)
    eng = pkg.Engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    inp, keep = world(torch, pkg, eng, grid, beams, landmarks=L, steps=frames)
    ses = pkg.PfSession(eng, n, L, sigma=bench.SIGMA, meas_var=bench.MEAS_VAR, score_gain=bench.SCORE_GAIN, seed=1234)
    if sweeps:
        ses.refine_set(STEPS[0], STEPS[1], sweeps)
    ses.reset(bench.true_pose(0))
    Lp = (L + 31) // 32 * 32
    m0 = torch.zeros((n, 5, Lp), device=dev)
    bench.fill_maps(torch, m0, inp["landmarks"], L, dev, n)
    ses.set_map_dev(m0, 5 * Lp, Lp)
    bench.settle(torch)
    times = []
    for k in range(frames):
        fr = inp["frames"][k % len(inp["frames"])]
        eng.scan_upload(fr["bx"], fr["by"])
        eng.obs_upload(fr["ids"], fr["zx"], fr["zy"], L)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ses.step(0, fr["dp"], True)
        b.record()
        torch.cuda.synchronize()
        if k >= 8:
            times.append(a.elapsed_time(b) * 1e3)
    ses.close()
    eng.close()
    return dict(what="session", particles=n, landmarks=L, grid=grid, beams=beams, sweeps=sweeps, frame_us=round(float(np.median(times)), 1),
                frames=len(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--skip-session", action="store_true")
    args = ap.parse_args()
    import torch

    pkg = load_package()
    for n, grid in ((65536, 1024), (1048576, 2048)):
        print(json.dumps(lattice_bench(torch, pkg, n, grid, 360, args.reps)), flush=True)
    if not args.skip_session:
        for sweeps in (0, 1, 2):
            print(json.dumps(session_bench(torch, pkg, 65536, 500, 1024, 360, sweeps)), flush=True)


if __name__ == "__main__":
    main()
