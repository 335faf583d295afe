"""The detector's specification (tests/_detect_spec.py) on hand-made scans, one per edge of the rule (tests/_detect_scenes.py):
what breaks, what counts, what is too wide, what is occluded, the segment across the end of the scan, NaN, the degenerate scans
and the cap of 64 detections.  No GPU."""
import numpy as np
import pytest

import _detect_scenes as S
import _detect_spec as D

F = np.float32
SCENES = S.scenarios()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenario(name):
    bx, by, kw, want = SCENES[name]
    zx, zy, ndet, stats = D.detect(bx, by, **kw)
    assert stats.tolist() == [want["segments"], want["accepted"], want["ndet"], 0], name
    assert ndet == want["ndet"] == min(want["accepted"], D.MAX_DETECTIONS)
    assert np.isfinite(zx).all() and np.isfinite(zy).all()
    assert not zx[ndet:].any() and not zy[ndet:].any()


def test_the_thresholds_sit_where_the_scenarios_say():
    """The scenarios' "equal" gaps are the thresholds themselves and their "above" gaps the next float32 up."""
    for name, thr in (("jump", S.JUMP * S.JUMP), ("width", S.WIDTH * S.WIDTH), ("guard", S.GUARD * S.GUARD)):
        d = S.just_over(thr)
        assert thr + d * d == np.nextafter(thr, F(np.inf)), name
    bx, by, _, _ = SCENES["jump_equal"]
    dx = bx[2] - bx[1]
    assert dx * dx == S.JUMP * S.JUMP and by[2] == by[1]
    bx, by, _, _ = SCENES["jump_above"]
    dx, dy = bx[2] - bx[1], by[2] - by[1]
    assert dx * dx + dy * dy == np.nextafter(S.JUMP * S.JUMP, F(np.inf))
    bx, by, _, _ = SCENES["width_above"]
    dx, dy = bx[3] - bx[1], by[3] - by[1]
    assert dx * dx + dy * dy == np.nextafter(S.WIDTH * S.WIDTH, F(np.inf))
    for name in ("left_guard_above", "right_guard_above"):
        bx, by, _, _ = SCENES[name]
        k = 2 if name.startswith("left") else 4       # f, or q: the gap to the point in front of it
        dx, dy = bx[k] - bx[k - 1], by[k] - by[k - 1]
        assert dx * dx + dy * dy == np.nextafter(S.GUARD * S.GUARD, F(np.inf)), name


def test_centroids():
    """Summed in segment order and divided once: jump_equal's pair, and the wrap segment's c0 c1 c2 c3 (the sum runs through P - 1
    into 0), which comes second because its start index is the higher one."""
    bx, by, kw, _ = SCENES["jump_equal"]
    zx, zy, ndet, _ = D.detect(bx, by, **kw)
    assert ndet == 1 and zx[0] == (bx[1] + bx[2]) / F(2) and zy[0] == F(0)
    bx, by, kw, _ = SCENES["wrap_segment"]
    zx, zy, ndet, _ = D.detect(bx, by, **kw)
    order = [7, 8, 0, 1]
    sx = bx[order[0]]
    for b in order[1:]:
        sx = sx + bx[b]
    assert ndet == 2 and zx[1] == sx / F(4) and zy[1] == F(5)
    assert zx[0] == ((bx[3] + bx[4]) + bx[5]) / F(3)
    # without wrap only the interior cluster is left, with the same bits
    zx0, zy0, n0, _ = D.detect(bx, by, **dict(kw, wrap=0))
    assert n0 == 1 and zx0[0] == zx[0] and zy0[0] == zy[0]


def test_many_keeps_the_first_64_by_start_index():
    bx, by, kw, _ = SCENES["many"]
    zx, zy, ndet, stats = D.detect(bx, by, **kw)
    assert ndet == 64 and stats.tolist() == [70, 70, 64, 0]
    want = np.array([(bx[2 * k] + bx[2 * k + 1]) / F(2) for k in range(64)], F)
    assert np.array_equal(zx, want) and np.all(zy == F(50))


def test_max_range_and_params():
    bx, by, kw, _ = SCENES["jump_equal"]
    assert D.detect(bx, by, **dict(kw, max_range=0.1))[2] == 0       # the centroid lies 0.15 m out
    assert D.detect(bx, by, **dict(kw, max_range=0.2))[2] == 1
    assert D.params_ok(D.DEFAULTS)
    for bad in (dict(jump=0.0), dict(jump=float("nan")), dict(guard=0.2), dict(max_width=float("inf")), dict(max_range=-1.0),
                dict(min_points=0), dict(min_points=5, max_points=4), dict(max_points=65), dict(wrap=2)):
        assert not D.params_ok(D.params(**bad)), bad


def test_pole_fields_exercise_the_rule():
    """The random fields the GPU test deals from: detections, rejected segments of every kind, a segment across the end."""
    bx, by, kw = S.pole_field(1024, 5)
    zx, zy, ndet, stats = D.detect(bx, by, **kw)
    assert 10 < stats[1] < stats[0] and ndet == min(stats[1], 64)
    assert D.detect(bx, by, **dict(kw, wrap=0))[3][1] == stats[1] - 1    # the pole across the end goes
    assert D.detect(bx, by, **dict(kw, guard=kw["jump"]))[3][1] > stats[1]   # ... and some poles are occluded
    assert D.detect(*S.pole_field(4096, 6)[:2], **kw)[3][1] > 64
