"""The fitted detector (tests/_detect_fit_spec.py) as a detector, on the scene, poses and drive of test_detect_behaviour_cpu.py
(restated here): it finds the poles the centroid detector finds, every one strictly closer to its pole's centre; a flat piece of
wall seen through a gap, which the centroid detector takes for a pole, it rejects; and the chain detect -> associate -> evidence
over the 40 noisy frames of the drive ends with one landmark per pole seen and a more accurate map.  No GPU."""
import numpy as np
import pytest

import _detect_fit_spec as DF
import _detect_spec as D
import _evidence_spec as E

RHO, HALF, NBEAMS = 0.1, 6.0, 360
FIT = (RHO, 0.0)
_rng = np.random.default_rng(3)
_ang = np.deg2rad(30.0 * np.arange(12) + _rng.uniform(-5, 5, 12))
_rad = _rng.uniform(2.5, 4.5, 12)
POLES = np.stack([_rad * np.cos(_ang), _rad * np.sin(_ang)], 1)
POSES = [(0.0, 0.0, 0.0), (0.4, -0.3, 0.2), (-0.5, 0.2, -0.4), (0.3, 0.5, 1.0), (-0.2, -0.6, 2.5)]


def to_world(pose, zx, zy):
    """w = t + R(theta)^T z (the update's own observed point)."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return pose[0] + c * zx + s * zy, pose[1] - s * zx + c * zy


def nearest_pole(pose, zx, zy):
    wx, wy = to_world(pose, zx.astype(np.float64), zy.astype(np.float64))
    d = np.hypot(wx[:, None] - POLES[None, :, 0], wy[:, None] - POLES[None, :, 1])
    return np.argmin(d, axis=1), d.min(axis=1)


@pytest.mark.parametrize("pose", POSES)
def test_every_fitted_detection_is_closer_to_its_pole(pose):
    bx, by, hit, _ = D.raycast(pose, POLES, RHO, HALF, NBEAMS)
    cx, cy, nc, cstats = D.detect(bx, by)
    zx, zy, nz, stats = DF.detect_fit(bx, by, FIT)
    who_c, dc = nearest_pole(pose, cx[:nc], cy[:nc])
    who_z, dz = nearest_pole(pose, zx[:nz], zy[:nz])
    print(f"pose {pose}: {nz} detections; centroid worst {dc.max():.4f} m, fit worst {dz.max():.4f} m; stats {stats.tolist()}")
    # the same poles, in the same (scan) order: no pole lost to the shape test, and — the centroid detector gives none — no wall
    assert nc >= 8 and who_z.tolist() == who_c.tolist() and stats[3] == 0 and stats[:3].tolist() == cstats[:3].tolist()
    assert len(set(who_z.tolist())) == nz
    assert np.all(dz < dc)


def test_an_empty_room_gives_nothing():
    for pose in POSES:
        bx, by, hit, _ = D.raycast(pose, POLES[:0], RHO, HALF, NBEAMS)
        assert np.all(hit == -1) and DF.detect_fit(bx, by, FIT)[2] == 0


def test_a_flat_piece_of_wall_behind_a_gap_is_rejected():
    """A wall 1.5 m in front of the sensor with a gap of 0.2 m, a second wall 3 m out: through the gap the beams see 0.4 m of the far
    wall, flanked by range jumps of more than guard — the centroid detector's rule has no means to tell it from a pole.  Its
    points lie on a line: s2 = w^2 / 12 for a width w, above rho^2 once w > 3.46 rho."""
    ang = np.deg2rad(np.arange(-60.5, 61.0, 1.0))                 # a sensor of 121 degrees: no wrap, the ends are cut
    y_near = 1.5 * np.tan(ang)
    rng_ = np.where(np.abs(y_near) < 0.1, 3.0, 1.5) / np.cos(ang)
    bx, by = (rng_ * np.cos(ang)).astype(np.float32), (rng_ * np.sin(ang)).astype(np.float32)
    piece = np.flatnonzero(np.abs(y_near) < 0.1)
    width = float(by[piece[-1]] - by[piece[0]])
    cx, cy, nc, _ = D.detect(bx, by, wrap=0)
    zx, zy, nz, stats = DF.detect_fit(bx, by, FIT, wrap=0)
    s2 = float(np.mean((bx[piece] - bx[piece].mean()) ** 2 + (by[piece] - by[piece].mean()) ** 2))
    print(f"{len(piece)} points, {width:.3f} m wide, s2 / rho2 = {s2 / RHO ** 2:.2f}")
    assert 0.35 < width <= 0.4 and len(piece) >= 3
    assert nc == 1 and abs(cx[0] - 3.0) < 1e-3 and abs(cy[0]) < 0.03
    assert nz == 0 and stats.tolist() == [3, 0, 0, 1]


# ------------------------------------------------------------------ the chain
N, SLOTS, FRAMES = 256, 16, 40
KW = dict(seed=5, sigma=(0.01, 0.01, 0.002), meas_var=2.5e-3, score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
DP = (0.02, 0.005, 0.005)
PRUNE = (1, 1, 8, 9.0)


def chain(mode):
    """The drive: the noise-free motion model from the origin, every frame ray-cast with 1 cm of range noise.  mode: "centroid",
    "fit", or "ideal": the loop is fed the centres of the poles the centroid detector found, each moved along its bearing by the
    mean noise of the beams that hit it.
    -> (row of the heaviest particle, the poles detected at least once, per-detection distances to the pole centres)."""
    pose, dets, seen, dist = np.zeros(3), [], set(), []
    for f in range(FRAMES):
        pose = pose + np.array(DP)
        bx, by, hit, added = D.raycast(pose, POLES, RHO, HALF, NBEAMS, noise=np.random.default_rng(100 + f))
        zx, zy, k, _ = DF.detect_fit(bx, by, FIT if mode == "fit" else None)
        zx, zy = zx[:k].copy(), zy[:k].copy()
        who, d = nearest_pole(pose, zx, zy)
        seen.update(who.tolist())
        dist += d.tolist()
        if mode == "ideal":
            c, s = np.cos(pose[2]), np.sin(pose[2])
            dd = POLES[who] - pose[:2]
            cx, cy = c * dd[:, 0] - s * dd[:, 1], s * dd[:, 0] + c * dd[:, 1]
            rr = np.hypot(cx, cy)
            shift = np.array([added[hit == j].mean() for j in who])
            zx, zy = (cx * (1 + shift / rr)).astype(np.float32), (cy * (1 + shift / rr)).astype(np.float32)
        dets.append((zx, zy))
    world = dict(x=np.zeros(N, np.float32), y=np.zeros(N, np.float32), th=np.zeros(N, np.float32), mp=np.zeros((N, 5, SLOTS), np.float32))
    world["mp"][:, 2] = -1.0
    out = E.frame_loop(world, N, FRAMES, dp=DP, detections=lambda f: dets[f], gate=GATE, new_gate=NEW_GATE, create=1, score=False,
                       prune=PRUNE, **KW)
    last = out[-1]
    k = int(np.flatnonzero(last["anc"] == np.argmax(last["logw"]))[0])   # (the heaviest particle survives the resample)
    return last["map"][k], seen, np.array(dist)


def map_error(row):
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen, None] - POLES[None, :, 0], row[1, seen, None] - POLES[None, :, 1])
    return np.argmin(d, axis=1), float(np.sqrt(np.mean(np.min(d, axis=1) ** 2)))


def test_the_chain_maps_the_poles_more_accurately(orc):
    """Measured on this drive (heaviest particle of the last frame, RMS distance of its landmarks to the pole centres):
    centroid 0.0888 m, fit 0.0355 m, ideal detections 0.0106 m; all three maps hold one landmark per pole seen,
    twelve of twelve.  Per detection over the 40 frames (420 of them): centroid 0.0802 m RMS (worst 0.0978), fit 0.0141 m RMS (worst 0.0362)."""
    res = {}
    for mode in ("centroid", "fit", "ideal"):
        row, seen, dist = chain(mode)
        who, rms = map_error(row)
        res[mode] = rms
        print(f"{mode}: {len(who)} landmarks, map rms {rms:.4f} m; {len(seen)} poles seen; {len(dist)} detections, "
              f"rms {np.sqrt(np.mean(dist ** 2)):.4f} m, worst {dist.max():.4f} m")
        assert len(seen) >= 10
        assert sorted(who.tolist()) == sorted(seen), mode
    assert res["fit"] < res["centroid"], res
