"""tests/_localise_miss_spec.py on the CPU: with the mode off its loop IS the two localise loops; every seen landmark within range
is accounted for exactly once; and each edge of the predicate sits where it claims — the range bound, the particle's own position,
the arc's bounds, a wrapping arc, the margin, the neighbour bin, an unseen slot, a NaN pose, no detections, everything matched."""
import numpy as np
import pytest

import _assoc_spec as A
import _fov_spec as V
import _localise_detcov_spec as LD
import _localise_miss_spec as MS
import _localise_spec as LS
import _sight_spec as S

F = np.float32
Q, GATE = 0.02, 9.21
INF = F(np.inf)


def one(mx, my, pose=(0.0, 0.0, 0.0), view_range=5.0, arc=None, T=None, margin=None, zx=(), zy=(), pxx=0.05):
    """The classes of ONE landmark under ONE pose -> (missed, spared, outside, matched) of particle 0."""
    M = np.array([[mx], [my], [pxx], [0.0], [0.05]], np.float32)
    x, y, th = (np.array([v], F) for v in pose)
    _, stats, _, missed, spared, outside = MS.localise(M, x, y, th, np.array(zx, F), np.array(zy, F), Q, GATE, 0.0, 0.0,
                                                        (view_range, arc, margin), T)
    return int(missed[0]), int(spared[0]), int(outside[0]), int(stats[0, 0])


def cloud_scene(seed, n=200, L=30, detcov=False):
    rng = np.random.default_rng(seed)
    M = np.zeros((5, L), np.float32)
    M[0], M[1] = rng.uniform(-8, 8, L), rng.uniform(-8, 8, L)
    M[2], M[4] = 0.2, 0.2
    M[2, rng.random(L) < 0.2] = -1.0
    truth = np.array([0.5, -0.3, 0.2])
    world = dict(x=(truth[0] + rng.normal(0, 0.5, n)).astype(F), y=(truth[1] + rng.normal(0, 0.5, n)).astype(F),
                 th=(truth[2] + rng.normal(0, 0.1, n)).astype(F))

    def detections(f):
        if f == 2:
            return None   # a frame without observations
        r = np.random.default_rng(100 * seed + f)
        seen = np.flatnonzero(~(M[2] < 0))
        dx, dy = M[0, seen] - truth[0], M[1, seen] - truth[1]
        near = np.hypot(dx, dy) < 6.0
        c, s = np.cos(truth[2]), np.sin(truth[2])
        zx = (c * dx[near] - s * dy[near] + r.normal(0, 0.02, near.sum())).astype(F)
        zy = (s * dx[near] + c * dy[near] + r.normal(0, 0.02, near.sum())).astype(F)
        if not detcov:
            return zx, zy
        k = len(zx)
        return zx, zy, (np.full(k, 0.02, F), np.full(k, 0.004, F), np.full(k, 0.03, F))

    return M, world, detections


@pytest.mark.parametrize("clutter", (0.0, -3.0))
def test_the_loop_with_the_mode_off_is_the_existing_loops(orc, clutter):
    n, frames = 200, 4
    kw = dict(seed=5, sigma=(0.05, 0.05, 0.02), score_gain=0.0, dp=np.array([0.1, 0.0, 0.02], F), gate=GATE, log_clutter=clutter,
              ess=0.5, score=False)
    for detcov in (False, True):
        M, world, det = cloud_scene(11, n, detcov=detcov)
        if detcov:
            want = LD.frame_loop(world, n, frames, detections=det, known_map=M, **kw)
            got = MS.frame_loop(world, n, frames, detections=det, known_map=M, miss=None, **kw)
        else:
            want = LS.frame_loop(world, n, frames, detections=det, known_map=M, meas_var=Q, **kw)
            got = MS.frame_loop(world, n, frames, detections=det, known_map=M, meas_var=Q, miss=None, **kw)
        for f, (g, w) in enumerate(zip(got, want)):
            for key in w:   # key by key, bit for bit
                if w[key] is None:
                    assert g[key] is None, (f, key)
                elif isinstance(w[key], np.ndarray):
                    assert g[key].dtype == w[key].dtype and np.array_equal(g[key].view(np.uint8), w[key].view(np.uint8)), (f, key)
                else:
                    assert g[key] == w[key], (f, key)
            assert g["missed"] is None and g["spared"] is None and g["outside"] is None


def test_every_seen_landmark_in_range_is_accounted_for_once(orc):
    M, world, det = cloud_scene(12, 300, 60)
    x, y, th = world["x"], world["y"], world["th"]
    zx, zy = det(0)
    rng = np.random.default_rng(3)
    ang = np.linspace(-np.pi, np.pi, 360, endpoint=False)
    rad = rng.uniform(1.0, 6.0, 360)
    T = S.table((rad * np.cos(ang)).astype(F), (rad * np.sin(ang)).astype(F), 64)
    view_range, arc = 5.5, (V.bound(-2.2), V.bound(2.2))   # a wrapping arc (lo > hi): blind behind
    assert arc[0] > arc[1]
    assoc, stats, _, missed, spared, outside = MS.localise(M, x, y, th, zx, zy, Q, GATE, 0.0, -1.0, (view_range, arc, 0.3), T)
    seen = ~(M[2] < 0)
    r2 = ((M[0][None] - x[:, None]) ** 2 + (M[1][None] - y[:, None]) ** 2).astype(F)
    in_range = seen[None] & (r2 <= F(view_range) * F(view_range))
    matched_in_range = (in_range & (assoc != A.NONE)).sum(axis=1)
    assert np.array_equal(missed + spared + outside + matched_in_range, in_range.sum(axis=1))
    assert missed.sum() > 0 and spared.sum() > 0 and outside.sum() > 0 and matched_in_range.sum() > 0


def test_the_range_bound_and_the_next_float_beyond(orc):
    r = F(5.0)
    assert F(r * r) == F(25.0)
    assert one(5.0, 0.0, view_range=5.0)[:3] == (1, 0, 0)          # r2 == view_range^2 exactly: in range
    assert one(np.nextafter(r, INF), 0.0, view_range=5.0)[:3] == (0, 0, 0)   # the next float beyond: r2 > view_range^2
    assert F(np.nextafter(r, INF)) ** 2 > F(25.0)


def test_the_particles_own_position_has_no_direction(orc):
    blind = (F(1.0), F(1.5))   # an arc that does not hold p = 0
    T = np.full(32, 0.01, F)   # something very near in every direction
    assert one(1.25, 3.5, pose=(1.25, 3.5, 0.7), arc=blind, T=T, margin=0.1)[:3] == (1, 0, 0)   # in view, never hidden
    assert one(3.0, 0.0, arc=blind)[:3] == (0, 0, 1)                                            # (the arc does exclude p = 0)


def test_a_direction_on_a_bound_is_in_view(orc):
    p = V.diamond(np.array([1.0], F), np.array([1.0], F))[0][0]   # the direction (1, 1): p = 0.5 exactly
    assert p == F(0.5)
    below, above = np.nextafter(p, F(0)), np.nextafter(p, F(4))
    assert one(1.0, 1.0, arc=(p, F(1.0)))[:3] == (1, 0, 0)        # on lo
    assert one(1.0, 1.0, arc=(F(0.0), p))[:3] == (1, 0, 0)        # on hi
    assert one(1.0, 1.0, arc=(above, F(1.0)))[:3] == (0, 0, 1)
    assert one(1.0, 1.0, arc=(F(0.0), below))[:3] == (0, 0, 1)


def test_a_wrapping_arc_and_the_whole_circle(orc):
    wrap = (F(3.0), F(1.0))   # through p = 4 = 0: ahead; blind from 1 to 3
    assert one(2.0, 0.0, arc=wrap)[:3] == (1, 0, 0)      # p = 0
    assert one(0.0, -2.0, arc=wrap)[:3] == (1, 0, 0)     # p = 3: on lo
    assert one(-2.0, 0.0, arc=wrap)[:3] == (0, 0, 1)     # p = 2: behind
    assert one(-2.0, 0.0, arc=MS.ALL)[:3] == (1, 0, 0)
    assert one(-2.0, 0.0, arc=None)[:3] == (1, 0, 0)


def test_the_margin_g_equal_to_zero_is_not_hidden(orc):
    T = np.full(32, 0.01, F)
    assert one(2.0, 0.0, T=T, margin=2.0)[:3] == (1, 0, 0)                       # g = r - margin == 0: not hidden
    assert one(2.0, 0.0, T=T, margin=float(np.nextafter(F(2.0), F(0))))[:3] == (1, 0, 0)   # g = one ulp, g^2 < near: in sight
    assert one(2.0, 0.0, T=T, margin=1.0)[:3] == (0, 1, 0)                       # g = 1, near = 0.01 < 1: hidden
    assert one(2.0, 0.0, T=np.full(32, INF, F), margin=1.0)[:3] == (1, 0, 0)     # nothing was hit: not hidden


def test_hidden_through_the_neighbour_bin_only(orc):
    j = int(S.bin_of(np.array([2.0], F), np.array([0.3], F), 32)[0][0])
    for d in (-1, 1):
        T = np.full(32, INF, F)
        T[(j + d) % 32] = 0.25
        assert one(2.0, 0.3, T=T, margin=0.5)[:3] == (0, 1, 0)
    T = np.full(32, INF, F)
    T[(j + 2) % 32] = T[(j - 2) % 32] = 0.25
    assert one(2.0, 0.3, T=T, margin=0.5)[:3] == (1, 0, 0)


def test_an_unseen_slot_and_a_nan_pose_count_nothing(orc):
    assert one(1.0, 0.0, pxx=-1.0)[:3] == (0, 0, 0)
    for pose in ((np.nan, 0.0, 0.0), (0.0, np.nan, 0.0)):
        assert one(1.0, 0.0, pose=pose, arc=(F(1.0), F(1.5)), T=np.full(32, 0.01, F), margin=0.1)[:3] == (0, 0, 0)
    # a heading that is not a number gives no direction: in view and not hidden, as in the evidence stage
    assert one(1.0, 0.0, pose=(0.0, 0.0, np.nan), arc=(F(1.0), F(1.5)), T=np.full(32, 0.01, F), margin=0.1)[:3] == (1, 0, 0)


def test_no_detections_and_every_landmark_matched(orc):
    M, world, det = cloud_scene(13, 1, 40)
    seen = ~(M[2] < 0)
    x, y, th = np.array([0.5], F), np.array([-0.3], F), np.array([0.2], F)
    none = np.zeros(0, F)
    _, stats, ll, missed, spared, outside = MS.localise(M, x, y, th, none, none, Q, GATE, 0.0, -2.0, (100.0, None, None))
    assert missed[0] == seen.sum() and spared[0] == 0 and outside[0] == 0          # K = 0: every visible landmark is missed
    assert ll[0] == F(seen.sum()) * F(-2.0)
    c, s = np.cos(0.2), np.sin(0.2)
    dx, dy = M[0, seen].astype(np.float64) - 0.5, M[1, seen].astype(np.float64) + 0.3
    zx, zy = (c * dx - s * dy).astype(F), (s * dx + c * dy).astype(F)
    assert len(zx) <= 64
    _, stats, _, missed, _, _ = MS.localise(M, x, y, th, zx, zy, Q, GATE, 0.0, -2.0, (100.0, None, None))
    assert stats[0, 0] == seen.sum() and missed[0] == 0                            # every landmark matched: none missed
