#!/usr/bin/env python3
"""profiles/detect_fit_measure.py kernel | session [N L STEPS ROUNDS] | ab PARENT_LIB [REPS] — the fitted detector on the GPU.
  kernel   one process: the detector's launch alone (SLAM_PROF_PAGES brackets) on random pole fields of 360, 1080 and 4096
           points, wrap on, in the variants the loaded library has — "centroid" (slam_detect_scan_dev), "fit NULL"
           (slam_detect_scan_fit_dev without a fit) and "fit" (radius 0.1) — the variants' rounds interleaved: per variant and
           size the median, minimum and maximum over the rounds of the mean time of REPS launches.  With SLAM_HIP_LIB naming a
           build of an earlier commit only "centroid" exists.  Ends with one line `RESULT {json}`.
  ab       runs `kernel` REPS times per library, this build and PARENT_LIB alternating, one fresh process each, and prints per
           size the centroid launch of both as median [min, max] over the processes' medians.
  session  ms_per_step (wall clock around scan upload + slam_pf_step + slam_pf_best, which waits for the frame) of an associating
           rows session of N x L in the pole room of tests/test_gpu_detect_fit_session.py, 360 beams, a different scan every
           frame: the fit on against the fit off, the two sessions' rounds interleaved in one process.
Measurement tooling: prints, asserts nothing about time.  Default session: 65 536 x 500, 40 steps per round, 5 rounds."""
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
mode = sys.argv[1] if len(sys.argv) > 1 else "kernel"
REPS, ROUNDS, DEV, FIT = 50, 7, "cuda:0", (0.1, 0.0)


def spread(t):
    return f"median {statistics.median(t):8.2f}   min {min(t):8.2f}   max {max(t):8.2f}"


if mode == "ab":
    parent, reps = sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 3
    res = {"this": [], "parent": []}
    for r in range(reps):
        for name in ("this", "parent"):
            env = dict(os.environ)
            if name == "parent":
                env["SLAM_HIP_LIB"] = parent
            out = subprocess.run([sys.executable, __file__, "kernel"], env=env, capture_output=True, text=True, timeout=120)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")]
            if out.returncode or not line:
                print(name, "FAILED", out.stderr[-400:], flush=True)
                sys.exit(1)
            res[name].append(json.loads(line[0][7:]))
    for P in ("360", "1080", "4096"):
        for name in ("parent", "this"):
            for variant in sorted(res[name][0][P]):
                print(f"P = {P:4s} {name:6s} {variant:9s} over {reps} processes, us: {spread([r[P][variant] for r in res[name]])}", flush=True)
    sys.exit(0)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import _detect_fit_spec as DF  # noqa: E402
import _detect_scenes as S  # noqa: E402
import _detect_spec as D  # noqa: E402
import __graft_entry__ as G  # noqa: E402

if mode == "kernel":
    lib_path = os.environ.get("SLAM_HIP_LIB") or str(G.PKG_DIR / "lib" / "libslam_hip.so")
    raw = C.CDLL(lib_path)
    pkg = G.load_package()
    missing = [k for k in pkg.SIGNATURES if not hasattr(raw, k)]
    for k in missing:                # a build of an earlier commit: bind what it has
        del pkg.SIGNATURES[k]
    has_fit = "slam_detect_scan_fit_dev" in pkg.SIGNATURES
    e = pkg.Engine(0)
    PAGES = pkg.Engine.PROF_PAGES
    print(f"{lib_path}: {'with' if has_fit else 'WITHOUT'} the fit; {ROUNDS} rounds x {REPS} launches per variant, interleaved; an empty "
          f"bracket measures {1e3 * e.profile_bracket_overhead():.2f} us")
    variants = {"centroid": lambda kw: e.detect_scan_dev(**kw)}
    if has_fit:
        variants["fit NULL"] = lambda kw: e.detect_scan_fit_dev(None, **kw)
        variants["fit"] = lambda kw: e.detect_scan_fit_dev(FIT, **kw)
    result = {}
    for P in (360, 1080, 4096):
        bx, by, kw = S.pole_field(P, 7)
        st = DF.detect_fit(bx, by, FIT, **kw)[3]
        e.scan_upload(bx, by)
        for v in variants.values():
            for _ in range(5):
                v(kw)
        e.detections()
        e.profile_enable(PAGES)
        e.profile_read(PAGES)
        t = {k: [] for k in variants}
        for _ in range(ROUNDS):
            for k, v in variants.items():
                for _ in range(REPS):
                    v(kw)
                ms, launches = e.profile_read(PAGES)
                assert launches == REPS
                t[k].append(1e3 * ms / launches)
        e.profile_enable()
        for k in variants:
            print(f"  P = {P:4d} {k:9s} us: {spread(t[k])}   (under the fit: {st[0]} segments, {st[1]} accepted, {st[3]} rejected by shape)")
        result[str(P)] = {k: statistics.median(v) for k, v in t.items()}
    e.close()
    print("RESULT " + json.dumps(result))
    sys.exit(0)

# ---- the session
import _shard_worker as W  # noqa: E402
import oracle  # noqa: E402

n, L, steps, rounds = (int(v) for v in (sys.argv[2:6] + ["65536", "500", "40", "5"][len(sys.argv) - 2:]))
pkg = G.load_package()
oracle.build(ref=False)
rng = np.random.default_rng(12)
POLES, RHO, HALF, DP = rng.uniform(-4.0, 4.0, (12, 2)), 0.1, 5.0, [0.01, -0.005, 0.002]
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
meta, edt, _, _, _ = W.make_world(L=0)
d_edt = torch.from_numpy(edt).to(DEV)
total = 10 + steps * rounds
scans = [D.raycast((f % 50 + 1) * np.array(DP), POLES, RHO, HALF, 360, noise=np.random.default_rng(900 + f))[:2] for f in range(total)]
print(f"{n} x {L} rows session, association on, 360 beams; {rounds} rounds x {steps} steps per session, rounds interleaved")


class Session:
    def __init__(self, fit):
        self.e = pkg.Engine(0)
        self.e.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
        self.ses = pkg.PfSession(self.e, n, L, map_layout="rows", **KW)
        self.ses.assoc_set(9.21, 50.0, True)
        self.ses.reset([0.0, 0.0, 0.0])
        self.ses.detect_fit_set(FIT if fit else None)
        self.t = []

    def step(self, f):
        self.e.scan_upload(*scans[f])
        self.ses.step(0, DP, True)
        return self.ses.best()

    def round(self, r):
        t0 = time.perf_counter()
        for f in range(10 + r * steps, 10 + (r + 1) * steps):
            self.step(f)
        self.t.append(1e3 * (time.perf_counter() - t0) / steps)


both = {"fit on": Session(True), "fit off": Session(False)}
for s in both.values():
    for f in range(10):
        s.step(f)
for r in range(rounds):
    for s in both.values():
        s.round(r)
for k, s in both.items():
    print(f"  ms_per_step, {k:8s}: {spread(s.t)} ms   detector launches {s.e.detect_count()}, of them fits {s.e.detect_fit_count()}")
    s.ses.close()
    s.e.close()
