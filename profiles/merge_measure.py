#!/usr/bin/env python3
"""profiles/merge_measure.py [N L ROUNDS REPS] — the merge stage (slam_landmark_merge_dev) on the GPU, through the package, in ONE
process.  Two scenes on the same particles, ancestors and K = 32 detections:
  * "no duplicates": every detection is the observation of one landmark, every other seen landmark is a pole of its own;
  * "a duplicate per detection": beside each observed landmark a second slot holds the same pole, 5 cm off — every anchor absorbs one.
Per scene, interleaved round by round and each timed by the events around its own launch (SLAM_PROF_PAGES):
  * slam_associate_detcov_dev — the kernel of the same shape (K x L pairs with a 2x2 inverse each), on the same rows,
  * slam_landmark_merge_dev with evidence — behind slam_ekf_update_assoc_dev, on the rows that launch wrote (which also puts the
    duplicates back for the next repetition), and the same without evidence.
Then a rows session of 4096 particles x 32 slots with association, pruning and the detector, frame by frame (wall clock, one
synchronisation per frame): merging never switched on (the parent's frame) against merging on.
Per variant the median, minimum and maximum over the rounds; the SPREAD of a variant is max - min.  Measurement tooling: prints,
asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), 6 rounds of 10 launches."""
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_package  # noqa: E402

n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "6", "10"][len(sys.argv) - 1:]))
Lp = (L + 31) // 32 * 32
DEV, Q, GATE, NEW_GATE, MERGE_GATE, CMAX, K = "cuda:0", 0.02, 9.21, 50.0, 30.0, 8, 32
pkg = load_package()
e = pkg.Engine(0)
e.set_stream(torch.cuda.current_stream().cuda_stream)
rng = np.random.default_rng(1)
assert L >= 2 * K
lm = np.stack(np.meshgrid(np.arange(-20, 20, 1.5), np.arange(-20, 20, 1.5)), -1).reshape(-1, 2)   # poles at least 1.5 m apart
lm = lm[rng.permutation(len(lm))[:L]].astype(np.float32)
x, y, th = (torch.as_tensor((s * rng.standard_normal(n)).astype(np.float32)).to(DEV) for s in (0.05, 0.05, 0.002))
heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
ids = rng.permutation(L - K)[:K]                      # the observed landmarks; slots L - K .. L - 1 hold the duplicates in scene 2
zx, zy = lm[ids, 0].copy(), lm[ids, 1].copy()         # (the pose is the origin, heading 0: z = m)
e.detections_upload(zx, zy)
e.detections_cov_upload(np.full(K, 0.03, np.float32), np.full(K, 0.005, np.float32), np.full(K, 0.015, np.float32))


def scene(duplicates):
    pts = lm.copy()
    if duplicates:
        pts[L - K:] = lm[ids] + np.float32(0.05)
    d_in = torch.empty((n, 5, Lp), device=DEV)
    d_in[:, 0, :L] = torch.as_tensor(pts[:, 0]).to(DEV) + 0.02 * torch.randn((n, L), device=DEV)
    d_in[:, 1, :L] = torch.as_tensor(pts[:, 1]).to(DEV) + 0.02 * torch.randn((n, L), device=DEV)
    d_in[:, 2], d_in[:, 3], d_in[:, 4] = 0.05, 0.01, 0.04
    d_in[:, :, L:] = 0.0
    d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
    e.associate_dev(d_in, 5 * Lp, Lp, L, x, y, th, anc, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, None)
    return d_in, d_assoc


d_out = torch.empty((n, 5, Lp), device=DEV)
d_scratch = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_ev = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_stats = torch.empty((n, 3), dtype=torch.int32, device=DEV)
SCENES = {"no duplicates": scene(False), "a duplicate per detection": scene(True)}
VARIANTS = ("slam_associate_detcov_dev", "slam_landmark_merge_dev with evidence", "slam_landmark_merge_dev without evidence")


def launch(variant, d_in, d_assoc):
    if variant == VARIANTS[0]:
        e.associate_detcov_dev(d_in, 5 * Lp, Lp, L, x, y, th, anc, n, GATE, NEW_GATE, 1, d_scratch, Lp, None)
        return
    e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, Q, d_assoc, Lp, None)
    e.landmark_merge_dev(d_out, 5 * Lp, Lp, L, n, d_assoc, Lp, d_ev if variant == VARIANTS[1] else None, Lp, CMAX, MERGE_GATE, d_stats)


def report(name, t):
    print(f"  {name:58s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   spread {max(t) - min(t):6.1f} us")
    return statistics.median(t)


print(f"{n} x {L} (plane stride {Lp}), {len(heads)} distinct ancestors, K = {K}; {rounds} rounds x {reps} launches")
for sname, (d_in, d_assoc) in SCENES.items():
    d_ev.fill_(3)
    for v in VARIANTS:
        for _ in range(3):
            launch(v, d_in, d_assoc)
    e.sync()
    st = d_stats.sum(dim=0).cpu().numpy() / n
    print(f"{sname}: per particle merged {st[0]:.2f}  refused {st[1]:.2f}  seen after {st[2]:.2f}")
    e.profile_enable(pkg.Engine.PROF_PAGES)
    times = {v: [] for v in VARIANTS}
    for _ in range(rounds):
        for v in VARIANTS:
            d_ev.fill_(3)
            for _ in range(reps):
                launch(v, d_in, d_assoc)
            e.sync()
            ms, launches = e.profile_read(pkg.Engine.PROF_PAGES)
            assert launches == reps
            times[v].append(1e3 * ms / launches)
    med = {v: report(v, t) for v, t in times.items()}
    print(f"  merge with evidence / detcov association: {med[VARIANTS[1]] / med[VARIANTS[0]]:.3f}")
    e.profile_enable()
e.close()
sys.stdout.flush()

# ---- a session frame: merging never switched on (the parent's frame) against merging on
sys.path.insert(0, str(ROOT / "tests"))
import _detect_spec as D  # noqa: E402
import _shard_worker as W  # noqa: E402

SN, SL, FRAMES, SROUNDS = 4096, 32, 20, 5
meta, edt, _, _, _ = W.make_world(L=SL)
d_edt = torch.from_numpy(edt).to(DEV)
angles = -2.351831 + 0.004363 * np.arange(1079)
poles = np.array([(-1.5, 2), (3, -2), (4, .6), (1, 3.5), (2.5, 3)], np.float64)
scans = [D.raycast((0.0, 0.03 * (f + 1), 0.0), poles, 0.1, 6.0, noise=np.random.default_rng(100 + f), angles=angles)[:2] for f in range(FRAMES)]


def session_frames(merge):
    eng = pkg.Engine(0)
    eng.grid_set_dev(0, d_edt, pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y))
    ses = pkg.PfSession(eng, SN, SL, map_layout="rows", seed=5, sigma=(0.005, 0.005, 0.001), meas_var=2.5e-3, score_gain=0.05)
    ses.assoc_set(GATE, NEW_GATE, True)
    mp = np.zeros((SN, 5, SL), np.float32)
    mp[:, 2] = -1.0
    ses.set_poses(np.zeros(SN, np.float32), np.zeros(SN, np.float32), np.zeros(SN, np.float32))
    ses.set_map(mp)
    ses.prune_set(1, 1, 8, 9.0)
    ses.detect_set(wrap=0)
    if merge:
        ses.merge_set(MERGE_GATE)
    t = []
    for f in range(FRAMES):
        eng.scan_upload(*scans[f])
        eng.sync()
        t0 = time.perf_counter()
        ses.step(0, [0.0, 0.03, 0.0], True)
        eng.sync()
        t.append(1e6 * (time.perf_counter() - t0))
    assert eng.merge_count() == (FRAMES if merge else 0)
    ses.close()
    eng.close()
    return statistics.median(t[5:])


print(f"session frame, {SN} x {SL} rows, association + pruning + detector (wrap = 0), 1079 beams; median of frames 5 .. {FRAMES - 1}, {SROUNDS} rounds:")
frames = {"merging never switched on": [], "merging on": []}
for _ in range(SROUNDS):
    for merge, name in zip((False, True), frames):
        frames[name].append(session_frames(merge))
for name, t in frames.items():
    report(name, t)
