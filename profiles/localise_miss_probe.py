#!/usr/bin/env python3
"""profiles/localise_miss_probe.py [N L ROUNDS REPS] — what counting the landmarks in view that no detection matched costs inside
the localise launch (slam_localise_miss_dev, slam_localise_detcov_miss_dev) against the launch without it (slam_localise_dev,
slam_localise_detcov_dev).  On the GPU, through the package, in ONE process, the scene of profiles/localise_probe.py.  Default
65 536 particles x 500 landmarks, K = 16 detections; 6 rounds of 20 launches, the variants interleaved round by round, each launch
timed by the events around it (SLAM_PROF_PAGES); one warm-up round first.

Variants, for each noise form: the stage as it was; the miss form with the range test only; with a field of view; with a field of
view and line of sight (a 1024-bin sight table of a synthetic scan).  Per variant the median, minimum and maximum over the rounds
and the ratio of its median to the stage's.  Measurement tooling: prints, asserts nothing about time (it does assert that every
miss variant leaves the stats and the log-likelihood's bits of the stage without misses)."""
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
VIEW_RANGE, MARGIN, BINS = 20.0, 0.5, 1024
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
zx, zy = (c * dx - s * dy).astype(np.float32), (s * dx + c * dy).astype(np.float32)
x = (true[0] + 0.3 * rng.standard_normal(n)).astype(np.float32)
y = (true[1] + 0.3 * rng.standard_normal(n)).astype(np.float32)
th = (true[2] + 0.03 * rng.standard_normal(n)).astype(np.float32)
ang = np.linspace(-np.pi, np.pi, 1080, endpoint=False)
rad = rng.uniform(5.0, 30.0, 1080)

e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
e.detections_upload(zx, zy)
e.detections_cov_upload(np.full(K, Q, np.float32), np.zeros(K, np.float32), np.full(K, Q, np.float32))
e.scan_upload((rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32))
e.sight_table_dev(BINS)
d_x, d_y, d_th = (torch.as_tensor(v).to(DEV) for v in (x, y, th))
d_M = torch.as_tensor(M).to(DEV)
d_prep = torch.empty((6, Lp), device=DEV)
e.known_map_prepare_dev(d_M, Lp, L, Q, d_prep)
lo, hi = float(pkg.fov_bound(-2.35)), float(pkg.fov_bound(2.35))   # 269.5 degrees, blind behind: a wrapping arc
VIEWS = {"range only": pkg.LocaliseView(VIEW_RANGE, 0.0, 4.0, 0, 0.0), "+ fov": pkg.LocaliseView(VIEW_RANGE, lo, hi, 0, 0.0),
         "+ fov + sight": pkg.LocaliseView(VIEW_RANGE, lo, hi, 1, MARGIN)}
out = {}


def buffers(name):
    out[name] = (torch.empty((n, 3), dtype=torch.int32, device=DEV), torch.empty((n,), device=DEV),
                 [torch.empty((n,), dtype=torch.int32, device=DEV) for _ in range(3)])
    return out[name]


def variants(form):
    plain, miss, d_map = ((e.localise_dev, e.localise_miss_dev, d_prep) if form == "iso" else
                          (e.localise_detcov_dev, e.localise_detcov_miss_dev, d_M))
    st, ll, _ = buffers(f"{form}: the stage")
    v = {f"{form}: the stage": lambda: plain(d_map, Lp, L, d_x, d_y, d_th, n, GATE, None, 0, st, ll)}
    for name, view in VIEWS.items():
        st2, ll2, cnt = buffers(f"{form}: miss, {name}")
        v[f"{form}: miss, {name}"] = (lambda st2=st2, ll2=ll2, cnt=cnt, view=view:
                                      miss(d_map, Lp, L, d_x, d_y, d_th, n, GATE, None, 0, st2, ll2, view, *cnt))
    return v


def timed(fn):
    e.profile_read(e.PROF_PAGES)
    for _ in range(reps):
        fn()
    e.sync()
    ms, cnt = e.profile_read(e.PROF_PAGES)
    assert cnt == reps
    return 1e3 * ms / cnt


run = {**variants("iso"), **variants("detcov")}
e.profile_enable(e.PROF_PAGES)
t = {k: [] for k in run}
for r in range(rounds + 1):   # (round 0: warm-up)
    for k, fn in run.items():
        a = timed(fn)
        if r:
            t[k].append(a)
e.profile_enable()
torch.cuda.synchronize()
print(f"n = {n}, L = {L} (plane stride {Lp}), K = {K}, view_range {VIEW_RANGE} m, {BINS} bins; {rounds} rounds of {reps} launches")
for form in ("iso", "detcov"):
    base = statistics.median(t[f"{form}: the stage"])
    st, ll, _ = out[f"{form}: the stage"]
    for k in run:
        if not k.startswith(form + ":"):
            continue
        v = t[k]
        line = (f"  {k:32s} median {statistics.median(v):9.1f} us   min {min(v):9.1f} us   max {max(v):9.1f} us   "
                f"spread {max(v) - min(v):7.1f} us   x {statistics.median(v) / base:5.3f}")
        if "miss" in k:
            st2, ll2, cnt = out[k]
            assert torch.equal(st, st2) and torch.equal(ll.view(torch.int32), ll2.view(torch.int32)), f"{k}: not the stage's bits"
            line += "   per particle: " + ", ".join(f"{nm} {c.float().mean().item():.1f}" for nm, c in zip(("missed", "spared", "outside"), cnt))
        print(line)
e.close()
