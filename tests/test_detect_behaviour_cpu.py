"""The detector (tests/_detect_spec.py) as a detector: a box room with twelve poles of radius 0.1 m, ray-cast in numpy at 360 beams.
Every pole that shows enough points and has no occluder beside it gives one detection inside its disc, walls give none; and the whole
chain on the spec loops — detect -> _assoc_spec -> _evidence_spec over a drive with range noise — ends with a map of exactly the
poles seen, as accurate as the same loop fed ideal detections, up to the pole's radius.  No GPU."""
import numpy as np
import pytest

import _detect_spec as D
import _evidence_spec as E

RHO, HALF, NBEAMS = 0.1, 6.0, 360
# one pole every 30 degrees (+-5) at 2.5 .. 4.5 m from the room's centre.  Seen from a pose within a metre of the centre two
# neighbouring poles are more than 10 degrees apart, so the piece of wall between them is wider than max_width (0.5 m): the rule
# cannot tell a NARROW piece of wall seen through a gap from a pole, and the scene has none.
_rng = np.random.default_rng(3)
_ang = np.deg2rad(30.0 * np.arange(12) + _rng.uniform(-5, 5, 12))
_rad = _rng.uniform(2.5, 4.5, 12)
POLES = np.stack([_rad * np.cos(_ang), _rad * np.sin(_ang)], 1)
POSES = [(0.0, 0.0, 0.0), (0.4, -0.3, 0.2), (-0.5, 0.2, -0.4), (0.3, 0.5, 1.0), (-0.2, -0.6, 2.5)]
P = D.DEFAULTS


def to_world(pose, zx, zy):
    """w = t + R(theta)^T z (the update's own observed point)."""
    c, s = np.cos(pose[2]), np.sin(pose[2])
    return pose[0] + c * zx + s * zy, pose[1] - s * zx + c * zy


def expected_poles(bx, by, hit):
    """From the geometry, not from the detector: the poles with at least min_points hits in one run of beams whose neighbours on
    both sides are no occluders (nearer than the run's end AND within guard of it)."""
    out = []
    x, y = bx.astype(np.float64), by.astype(np.float64)
    r = np.hypot(x, y)
    for k in range(len(POLES)):
        b = np.flatnonzero(hit == k)
        if len(b) < P["min_points"]:
            continue
        first = next(i for i in b if hit[i - 1] != k)                       # cyclic: the run may pass through beam 0
        run = (first + np.arange(len(b))) % NBEAMS
        if not np.all(hit[run] == k):
            continue                                                        # split by something in front of it
        f, e, p, q = run[0], run[-1], (run[0] - 1) % NBEAMS, (run[-1] + 1) % NBEAMS
        left = np.hypot(x[p] - x[f], y[p] - y[f]) <= P["guard"] and r[p] < r[f]
        right = np.hypot(x[q] - x[e], y[q] - y[e]) <= P["guard"] and r[q] < r[e]
        if not (left or right):
            out.append(k)
    return out


@pytest.mark.parametrize("pose", POSES)
def test_poles_are_detected_and_walls_are_not(pose):
    bx, by, hit, _ = D.raycast(pose, POLES, RHO, HALF, NBEAMS)
    zx, zy, ndet, stats = D.detect(bx, by)
    want = expected_poles(bx, by, hit)
    wx, wy = to_world(pose, zx[:ndet].astype(np.float64), zy[:ndet].astype(np.float64))
    d = np.hypot(wx[:, None] - POLES[None, :, 0], wy[:, None] - POLES[None, :, 1])
    who = np.argmin(d, axis=1)
    print(f"pose {pose}: {ndet} detections of {len(want)} expected poles, {stats[0]} segments, farthest {d.min(axis=1).max():.4f} m from its centre")
    assert len(want) >= 8                                  # the scene shows most of its poles from every pose
    assert sorted(who.tolist()) == sorted(want)            # one detection per such pole, and nothing else: no wall
    # every returned point lies on the pole's circle, so their centroid lies in its disc (1e-5: the float32 points and sums)
    assert np.all(d.min(axis=1) <= RHO + 1e-5)


def test_an_empty_room_gives_nothing():
    for pose in POSES:
        bx, by, hit, _ = D.raycast(pose, POLES[:0], RHO, HALF, NBEAMS)
        assert np.all(hit == -1)
        assert D.detect(bx, by)[2] == 0


# ------------------------------------------------------------------ the chain
N, SLOTS, FRAMES = 256, 16, 40
KW = dict(seed=5, sigma=(0.01, 0.01, 0.002), meas_var=2.5e-3, score_gain=1.0)
GATE, NEW_GATE = 9.21, 50.0
DP = (0.02, 0.005, 0.005)
PRUNE = (1, 1, 8, 9.0)


def chain(ideal):
    """The drive: the noise-free motion model from the origin, every frame ray-cast with 1 cm of range noise.  ideal: the loop is fed
    the centres of the poles the detector found, each moved along its bearing by the mean noise of the beams that hit it.
    -> (row of the heaviest particle, its evidence, the poles detected at least once)."""
    pose, dets, seen = np.zeros(3), [], set()
    for f in range(FRAMES):
        pose = pose + np.array(DP)
        bx, by, hit, added = D.raycast(pose, POLES, RHO, HALF, NBEAMS, noise=np.random.default_rng(100 + f))
        zx, zy, k, _ = D.detect(bx, by)
        zx, zy = zx[:k].copy(), zy[:k].copy()
        wx, wy = to_world(pose, zx.astype(np.float64), zy.astype(np.float64))
        who = np.argmin(np.hypot(wx[:, None] - POLES[None, :, 0], wy[:, None] - POLES[None, :, 1]), axis=1)
        seen.update(who.tolist())
        if ideal:
            c, s = np.cos(pose[2]), np.sin(pose[2])
            d = POLES[who] - pose[:2]
            cx, cy = c * d[:, 0] - s * d[:, 1], s * d[:, 0] + c * d[:, 1]
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
    return last["map"][k], last["ev"][k], seen


def map_error(row):
    seen = np.flatnonzero(~(row[2] < 0))
    d = np.hypot(row[0, seen, None] - POLES[None, :, 0], row[1, seen, None] - POLES[None, :, 1])
    return np.argmin(d, axis=1), float(np.sqrt(np.mean(np.min(d, axis=1) ** 2)))


def test_the_chain_maps_exactly_the_poles_seen(orc):
    """Measured on this drive (heaviest particle of the last frame, RMS distance of its landmarks to the pole centres):
    detector 0.0888 m, ideal detections 0.0106 m; both maps hold one landmark per pole seen, twelve of twelve."""
    row, _, seen = chain(ideal=False)
    who, rms = map_error(row)
    ideal_row, _, _ = chain(ideal=True)
    ideal_who, ideal_rms = map_error(ideal_row)
    print(f"detector: {len(who)} landmarks, rms {rms:.4f} m; ideal detections: {len(ideal_who)} landmarks, rms {ideal_rms:.4f} m; "
          f"{len(seen)} poles seen")
    assert len(seen) >= 10
    assert sorted(who.tolist()) == sorted(seen) and sorted(ideal_who.tolist()) == sorted(seen)
    # the detector's point is the centroid of the arc it sees: inside the disc, up to rho from the centre the ideal loop is given
    assert rms <= ideal_rms + RHO, (rms, ideal_rms)
