"""Does a filter that has to find its correspondences itself (tests/_assoc_spec.py: frame_loop) build the map the
known-correspondence filter builds?  A short synthetic drive on the CPU, no GPU and no grid (the scan-match score is zero: the
landmarks alone weigh the particles), in the mould of test_filter_behaviour_cpu.py."""
import numpy as np

import _assoc_spec as A

N, L_TRUE, SLOTS, FRAMES = 256, 12, 16, 40
KW = dict(seed=5, sigma=(0.01, 0.01, 0.002), meas_var=2.5e-3, score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
DP = (0.05, 0.01, 0.01)
NOISE = 0.03           # metres per axis on every detection
MISSED = 0.2


def drive():
    """12 landmarks at least 2 m apart, the true trajectory (the noise-free motion model from the origin), and per frame the
    true ids seen (20 % missed) with their noisy sensor-frame observations."""
    rng = np.random.default_rng(42)
    lm = []
    while len(lm) < L_TRUE:
        p = rng.uniform(-6, 6, 2)
        if all(np.hypot(*(p - o)) >= 2.0 for o in lm):
            lm.append(p)
    lm = np.array(lm)
    pose, frames = np.zeros(3), []
    for f in range(FRAMES):
        pose = pose + np.array(DP)
        c, s = np.cos(pose[2]), np.sin(pose[2])
        d = lm - pose[:2]
        z = np.stack([c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]], axis=1) + NOISE * rng.standard_normal((L_TRUE, 2))
        ids = np.flatnonzero(rng.random(L_TRUE) >= MISSED).astype(np.int32)
        frames.append((ids, z[ids, 0].astype(np.float32), z[ids, 1].astype(np.float32), rng.permutation(len(ids))))
    return lm, frames


def yardstick(orc, frames):
    """The same drive through the oracle's stages with the true ids: landmark id -> slot id."""
    x = y = th = np.zeros(N, np.float32)
    mp = np.zeros((N, 5, SLOTS), np.float32)
    mp[:, 2] = -1.0
    anc = None
    for f, (ids, zx, zy, _) in enumerate(frames):
        x, y, th = orc.motion_sample(x, y, th, anc, N, 0, DP, KW["sigma"], KW["seed"], f)
        mp, ll = orc.ekf_update(mp, x, y, th, anc, ids, zx, zy, KW["meas_var"])
        logw, m = orc.logweight_carry(np.zeros(N, np.float32), ll, KW["score_gain"], None)
        wq, _ = orc.quantise_weights(logw, m)
        anc = orc.resample(wq, KW["seed"], f)
    return mp[int(np.argmax(logw))]


def map_error(row, lm):
    """-> (seen slots, distinct true landmarks they are nearest to, RMS distance to those)."""
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen, None] - lm[None, :, 0], row[1, seen, None] - lm[None, :, 1])
    return len(seen), len(np.unique(np.argmin(d, axis=1))), float(np.sqrt(np.mean(np.min(d, axis=1) ** 2)))


def test_the_map_grown_from_nothing_matches_the_known_correspondence_map(orc):
    """Measured on this drive (heaviest particle of the last frame, RMS distance of its landmarks to the truth):
    known correspondences 0.0241 m, associating filter 0.0231 m; both hold exactly one landmark per true landmark."""
    lm, frames = drive()
    ref_row = yardstick(orc, frames)
    ref_seen, ref_distinct, ref_rms = map_error(ref_row, lm)
    # the yardstick itself converges on this scene: every landmark found, well inside the detection noise after ~32 sightings
    assert ref_seen == ref_distinct == L_TRUE and ref_rms < NOISE, (ref_seen, ref_distinct, ref_rms)

    world = dict(x=np.zeros(N, np.float32), y=np.zeros(N, np.float32), th=np.zeros(N, np.float32), mp=np.zeros((N, 5, SLOTS), np.float32))
    world["mp"][:, 2] = -1.0
    out = A.frame_loop(world, N, FRAMES, dp=DP, detections=lambda f: (frames[f][1][frames[f][3]], frames[f][2][frames[f][3]]),
                       gate=GATE, new_gate=NEW_GATE, create=1, score=False, **KW)
    last = out[-1]
    row = last["map"][int(np.flatnonzero(last["anc"] == np.argmax(last["logw"]))[0])]   # (the heaviest particle survives the resample)
    seen, distinct, rms = map_error(row, lm)
    print(f"known correspondences: rms {ref_rms:.4f} m; associating: rms {rms:.4f} m, {seen} landmarks")
    assert seen == distinct == L_TRUE, (seen, distinct)
    # The two filters differ in slot order and summation rounding only: beyond a factor of two lies a wrong association, not noise.
    assert rms <= 2.0 * ref_rms, (rms, ref_rms)
