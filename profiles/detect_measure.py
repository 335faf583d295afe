#!/usr/bin/env python3
"""profiles/detect_measure.py [N L STEPS ROUNDS] — the landmark detector on the GPU, through the package, in ONE process:
  * slam_detect_scan_dev alone (SLAM_PROF_PAGES brackets) on random pole fields of 360, 1080 and 4096 points, wrap on: REPS
    launches per round, per size the median, minimum and maximum over the rounds of the mean launch time, beside the time an
    empty bracket measures;
  * ms_per_step (wall clock around scan upload + slam_pf_step + slam_pf_best, which waits for the frame) of an associating rows
    session of N particles x L landmark slots in the pole room of tests/test_gpu_detect_session.py, 360 beams, a different scan
    every frame — once with the detector on (slam_pf_detect_set), once fed the SAME detections through
    slam_detections_upload_host (made beforehand by tests/_detect_spec.py: the path that exists without the detector).  The two
    sessions are checked to end on the same bits.
Measurement tooling: prints, asserts nothing about time.  Default: 65 536 x 500, 40 steps per round, 5 rounds."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import _detect_scenes as S  # noqa: E402
import _detect_spec as D  # noqa: E402
import _shard_worker as W  # noqa: E402
from __graft_entry__ import load_package  # noqa: E402

n, L, steps, rounds = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "40", "5"][len(sys.argv) - 1:]))
REPS, DEV = 50, "cuda:0"
pkg = load_package()
PAGES = pkg.Engine.PROF_PAGES


def report(name, t, unit="us"):
    print(f"  {name:52s} median {statistics.median(t):9.2f} {unit}   min {min(t):9.2f} {unit}   max {max(t):9.2f} {unit}")


# ---- the kernel alone
e = pkg.Engine(0)
print(f"slam_detect_scan_dev alone, {rounds} rounds x {REPS} launches; an empty bracket measures {1e3 * e.profile_bracket_overhead():.2f} us")
for P in (360, 1080, 4096):
    bx, by, kw = S.pole_field(P, 7)
    st = D.detect(bx, by, **kw)[3]
    e.scan_upload(bx, by)
    for _ in range(5):
        e.detect_scan_dev(**kw)
    e.detections()
    e.profile_enable(PAGES)
    e.profile_read(PAGES)
    t = []
    for _ in range(rounds):
        for _ in range(REPS):
            e.detect_scan_dev(**kw)
        ms, launches = e.profile_read(PAGES)
        assert launches == REPS
        t.append(1e3 * ms / launches)
    e.profile_enable()
    report(f"P = {P:4d} ({st[0]} segments, {st[1]} accepted, {st[2]} written)", t)
e.close()

# ---- the session
import oracle  # noqa: E402

oracle.build(ref=False)
rng = np.random.default_rng(12)
POLES, RHO, HALF, DP = rng.uniform(-4.0, 4.0, (12, 2)), 0.1, 5.0, [0.01, -0.005, 0.002]
KW = dict(seed=77, sigma=(0.02, 0.02, 0.004), meas_var=0.02, score_gain=0.05)
meta, edt, _, _, _ = W.make_world(L=0)
d_edt = torch.from_numpy(edt).to(DEV)
total = 10 + steps * rounds
scans = [D.raycast((f % 50 + 1) * np.array(DP), POLES, RHO, HALF, 360, noise=np.random.default_rng(900 + f))[:2] for f in range(total)]
dets = []
for bx, by in scans:
    zx, zy, k, _ = D.detect(bx, by)
    dets.append((zx[:k].copy(), zy[:k].copy()))
print(f"{n} x {L} rows session, association on, 360 beams, {statistics.mean(len(d[0]) for d in dets):.1f} detections per frame; "
      f"{rounds} rounds x {steps} steps")


def session(detector):
    e = pkg.Engine(0)
    e.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    ses = pkg.PfSession(e, n, L, map_layout="rows", **KW)
    ses.assoc_set(9.21, 50.0, True)
    ses.reset([0.0, 0.0, 0.0])
    if detector:
        ses.detect_set()

    def step(f):
        e.scan_upload(*scans[f])
        if not detector:
            e.detections_upload(*dets[f])
        ses.step(0, DP, True)
        return ses.best()

    for f in range(10):
        step(f)
    t = []
    for r in range(rounds):
        t0 = time.perf_counter()
        for f in range(10 + r * steps, 10 + (r + 1) * steps):
            last = step(f)
        t.append(1e3 * (time.perf_counter() - t0) / steps)
    sel = np.arange(0, n, max(1, n // 64), dtype=np.int32)
    out = (last[0], ses.map_rows(sel), e.detect_count())
    ses.close()
    e.close()
    return t, out


t_on, out_on = session(True)
t_off, out_off = session(False)
report("ms_per_step, detector on (slam_pf_detect_set)", t_on, "ms")
report("ms_per_step, detections uploaded from the host", t_off, "ms")
same = np.array_equal(out_on[0].view(np.uint32), out_off[0].view(np.uint32)) and np.array_equal(out_on[1].view(np.uint32), out_off[1].view(np.uint32))
print(f"  detector launches: {out_on[2]} against {out_off[2]}; the two sessions end on the same bits: {same}")
