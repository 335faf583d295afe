#!/usr/bin/env python3
"""profiles/fov_measure.py [N L ROUNDS REPS [LIBDIR ...]] — the existence-evidence stage with a field of view on the GPU, through the package, in
ONE process, on the scene and the shape of profiles/sight_measure.py.  Behind the same slam_ekf_update_assoc_dev, on the rows that
launch wrote, through the same ancestors, table and evidence, interleaved round by round (SLAM_PROF_PAGES around each stage):
  * slam_landmark_evidence_dev                       — the plain stage (unchanged by the field of view: the parent of the next two),
  * slam_landmark_evidence_fov_dev use_sight = 0     — with everything in view (lo = 0, hi = 4: the parent's work plus the test),
  * ... and with the reference sensor's arc (1079 beams from -2.351831 rad in steps of 0.004363 rad, edge 0.1: it wraps),
  * slam_landmark_evidence_sight_dev                 — the sight stage (128 bins, margin 0.3; the parent of the next two),
  * slam_landmark_evidence_fov_dev use_sight = 1     — with everything in view, and with the sensor's arc.
Then a rows session of 4096 particles x 32 slots with association, pruning and the detector, frame by frame (wall clock, one
synchronisation per frame): one that never heard of the field of view against one in which it was switched on and off again.
Per variant the median, minimum and maximum over the rounds; the SPREAD of a variant is max - min.  Measurement tooling: prints,
asserts nothing about time.  Default: 65 536 x 500 (plane stride 512), 6 rounds of 10 pairs.
LIBDIR ...: builds of the library to compare (directories beside the package's lib/, e.g. lib_parent lib, as
make -C csrc OUT=../lib_parent leaves them): every build is loaded into this one process, each with an engine of its own on the
same stream and the same buffers, and every variant runs build after build inside each round.  None: the product's lib/."""
import importlib.util
import os
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from __graft_entry__ import PKG_DIR, load_package  # noqa: E402


def load_build(libdir):
    """The package once more under a name of its own, bound to PKG_DIR / libdir / libslam_hip.so."""
    os.environ["SLAM_HIP_LIB"] = str(PKG_DIR / libdir / "libslam_hip.so")
    name = "slam_build_" + libdir
    spec = importlib.util.spec_from_file_location(name, PKG_DIR / "__init__.py", submodule_search_locations=[str(PKG_DIR)])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    del os.environ["SLAM_HIP_LIB"]
    return mod


n, L, rounds, reps = (int(v) for v in (sys.argv[1:5] + ["65536", "500", "6", "10"][min(len(sys.argv), 5) - 1:]))
BUILDS = {d: load_build(d) for d in sys.argv[5:]} or {"lib": load_package()}
Lp = (L + 31) // 32 * 32
DEV, Q, GATE, NEW_GATE = "cuda:0", 0.02, 9.21, 50.0
HIT, MISS, CMAX, RANGE = 1, 1, 8, 15.0
BINS, MARGIN, NBEAMS = 128, 0.3, 360
pkg = next(iter(BUILDS.values()))
ANGLE_MIN, ANGLE_MAX, EDGE = np.float32(-2.351831), np.float32(-2.351831 + 0.004363 * 1078), np.float32(0.1)
ARC = (float(pkg.fov_bound(float(ANGLE_MIN + EDGE))), float(pkg.fov_bound(float(ANGLE_MAX - EDGE))))
ENGINES = {b: m.Engine(0) for b, m in BUILDS.items()}
for eng in ENGINES.values():
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
e = next(iter(ENGINES.values()))   # (the scene is made once, by the first build)
rng = np.random.default_rng(1)
lm = rng.uniform(-20, 20, (L, 2)).astype(np.float32)
x, y, th = (torch.as_tensor((s * rng.standard_normal(n)).astype(np.float32)).to(DEV) for s in (0.05, 0.05, 0.002))
heads = np.sort(rng.choice(n, max(1, n * 6 // 100), replace=False))
anc = torch.as_tensor(np.sort(heads[rng.integers(0, len(heads), n)]).astype(np.int32)).to(DEV)
d_in = torch.empty((n, 5, Lp), device=DEV)
d_in[:, 0, :L] = torch.as_tensor(lm[:, 0]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 1, :L] = torch.as_tensor(lm[:, 1]).to(DEV) + 0.05 * torch.randn((n, L), device=DEV)
d_in[:, 2], d_in[:, 3], d_in[:, 4] = 0.05, 0.01, 0.04
d_in[:, 2, :L][torch.rand((n, L), device=DEV) < 0.1] = -1.0
d_in[:, :, L:] = 0.0
d_out = torch.empty((n, 5, Lp), device=DEV)
d_assoc = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_ev_in = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_ev_out = torch.empty((n, Lp), dtype=torch.uint8, device=DEV)
d_stats = torch.empty((n, 2), dtype=torch.int32, device=DEV)
d_spared = torch.zeros((n,), dtype=torch.int32, device=DEV)
d_outside = torch.zeros((n,), dtype=torch.int32, device=DEV)
K = min(56, L)
ids = rng.permutation(L)[:K]
zx = np.concatenate([lm[ids, 0], rng.uniform(-20, 20, 8).astype(np.float32)])   # (the pose is the origin, heading 0: z = m)
zy = np.concatenate([lm[ids, 1], rng.uniform(-20, 20, 8).astype(np.float32)])
for eng in ENGINES.values():
    eng.detections_upload(zx, zy)
ang = -np.pi + 2 * np.pi * np.arange(NBEAMS) / NBEAMS
rad = rng.uniform(8.0, 20.0, NBEAMS)
for eng in ENGINES.values():
    eng.scan_upload((rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32))
    eng.sight_table_dev(BINS)
e.associate_dev(d_in, 5 * Lp, Lp, L, x, y, th, anc, n, Q, GATE, NEW_GATE, 1, d_assoc, Lp, None)
e.evidence_init_dev(d_in, 5 * Lp, Lp, L, n, d_ev_in, Lp, 3)
d_ev_in = torch.minimum(d_ev_in, torch.randint(0, 4, (n, Lp), dtype=torch.uint8, device=DEV))

# name -> (stage, bounds)
VARIANTS = {
    "slam_landmark_evidence_dev": ("plain", None),
    "slam_landmark_evidence_fov_dev use_sight=0, all in view": ("fov0", (0.0, 4.0)),
    "slam_landmark_evidence_fov_dev use_sight=0, sensor arc": ("fov0", ARC),
    "slam_landmark_evidence_sight_dev": ("sight", None),
    "slam_landmark_evidence_fov_dev use_sight=1, all in view": ("fov1", (0.0, 4.0)),
    "slam_landmark_evidence_fov_dev use_sight=1, sensor arc": ("fov1", ARC),
}


def pair(e, stage, bounds):
    e.ekf_update_assoc_dev(d_in, d_out, 5 * Lp, Lp, L, x, y, th, anc, n, Q, d_assoc, Lp, None)
    head = (d_out, 5 * Lp, Lp, L, x, y)
    tail = (anc, n, d_assoc, Lp, d_ev_in, d_ev_out, Lp, HIT, MISS, CMAX, RANGE)
    if stage == "plain":
        e.landmark_evidence_dev(*head, *tail, d_stats)
    elif stage == "sight":
        e.landmark_evidence_sight_dev(*head, th, *tail, MARGIN, d_stats, d_spared)
    else:
        e.landmark_evidence_fov_dev(*head, th, *tail, MARGIN, bounds[0], bounds[1], stage == "fov1", d_stats, d_spared, d_outside)


def report(name, t):
    print(f"  {name:58s} median {statistics.median(t):8.1f} us   min {min(t):8.1f} us   max {max(t):8.1f} us   spread {max(t) - min(t):6.1f} us")
    return statistics.median(t)


print(f"{n} x {L} (plane stride {Lp}), {len(heads)} distinct ancestors, K = {len(zx)}, {NBEAMS} beams, {BINS} bins; {rounds} rounds x {reps} pairs; "
      f"sensor arc lo = {ARC[0]:.6f}, hi = {ARC[1]:.6f}")
for name, (stage, bounds) in VARIANTS.items():
    for b, eng in ENGINES.items():
        d_spared.zero_()
        d_outside.zero_()
        for _ in range(5):
            pair(eng, stage, bounds)
        eng.sync()
        st = d_stats.sum(dim=0).cpu().numpy() / n
        print(f"      {b}: {name}: per particle pruned {st[0]:.2f}  seen after pruning {st[1]:.2f}  spared {d_spared.sum().item() / n:.2f}  "
              f"outside {d_outside.sum().item() / n:.2f}")
for eng in ENGINES.values():
    eng.profile_enable(pkg.Engine.PROF_EKF, pkg.Engine.PROF_PAGES)
times = {b: {name: [] for name in VARIANTS} for b in BUILDS}
update = {b: [] for b in BUILDS}
for _ in range(rounds):
    for name, (stage, bounds) in VARIANTS.items():
        for b, eng in ENGINES.items():   # build after build on the same rows: never one build's block of rounds against another's
            for _ in range(reps):
                pair(eng, stage, bounds)
            eng.sync()
            ms, launches = eng.profile_read(pkg.Engine.PROF_PAGES)
            assert launches == reps
            times[b][name].append(1e3 * ms / launches)
            ms, launches = eng.profile_read(pkg.Engine.PROF_EKF)
            update[b].append(1e3 * ms / launches)
names = list(VARIANTS)
for b, eng in ENGINES.items():
    print(f" build {b}:")
    report("slam_ekf_update_assoc_dev in front of each", update[b])
    med = {name: report(name, t) for name, t in times[b].items()}
    print(f"  fov use_sight=0 all in view / plain stage: {med[names[1]] / med[names[0]]:.3f}; sensor arc / plain stage: {med[names[2]] / med[names[0]]:.3f}")
    print(f"  fov use_sight=1 all in view / sight stage: {med[names[4]] / med[names[3]]:.3f}; sensor arc / sight stage: {med[names[5]] / med[names[3]]:.3f}")
    eng.profile_enable()
    eng.close()
sys.stdout.flush()

# ---- a session frame with the feature off: never switched on against switched on and off again
sys.path.insert(0, str(ROOT / "tests"))
import _detect_spec as D  # noqa: E402
import _shard_worker as W  # noqa: E402

SN, SL, FRAMES, SROUNDS = 4096, 32, 20, 5
meta, edt, _, _, _ = W.make_world(L=SL)
d_edt = torch.from_numpy(edt).to(DEV)
angles = -2.351831 + 0.004363 * np.arange(1079)
poles = np.array([(-1.5, 2), (3, -2), (4, .6), (1, 3.5), (2.5, 3)], np.float64)
scans = [D.raycast((0.0, 0.03 * (f + 1), 0.0), poles, 0.1, 6.0, noise=np.random.default_rng(100 + f), angles=angles)[:2] for f in range(FRAMES)]


def session_frames(pkg, ask):
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
    if ask:
        ses.prune_fov_set(True, float(ANGLE_MIN), float(ANGLE_MAX), float(EDGE))
        ses.prune_fov_set(False)
    t = []
    for f in range(FRAMES):
        eng.scan_upload(*scans[f])
        eng.sync()
        t0 = time.perf_counter()
        ses.step(0, [0.0, 0.03, 0.0], True)
        eng.sync()
        t.append(1e6 * (time.perf_counter() - t0))
    assert eng.fov_counts() == 0
    ses.close()
    eng.close()
    return statistics.median(t[5:])


print(f"session frame, {SN} x {SL} rows, association + pruning + detector (wrap = 0), 1079 beams; median of frames 5 .. {FRAMES - 1}, {SROUNDS} rounds:")
frames = {b: {"never switched on": [], "switched on and off again": []} for b in BUILDS}
for _ in range(SROUNDS):
    for ask, name in zip((False, True), ("never switched on", "switched on and off again")):
        for b, m in BUILDS.items():
            frames[b][name].append(session_frames(m, ask))
for b in BUILDS:
    for name, t in frames[b].items():
        report(f"{b}: {name}", t)
