"""Hand-made scans, one per edge of the detector's rule (tests/_detect_spec.py), and random pole fields.  TEST INFRASTRUCTURE
shared by test_detect_spec_cpu.py (which checks what the specification makes of each) and test_gpu_detect.py (which runs the kernel
on the same scans).

The critical pair of points of a scenario sits at the origin of an axis, so that the differences the rule forms are exact and a gap
can be placed ON a threshold or one float32 above it.  Isolated SEPARATOR points, 10 m from everything, close the scenario off: each
is a segment of one point (rejected wherever min_points >= 2) and too far away to occlude anything."""
import numpy as np

import _detect_spec as D

F = np.float32
# min_points = 2: a separator alone is no detection; max_range out of the way
KW = dict(jump=0.3, guard=1.0, max_width=0.5, max_range=1000.0, min_points=2, max_points=4, wrap=1)
JUMP, GUARD, WIDTH = F(KW["jump"]), F(KW["guard"]), F(KW["max_width"])


def just_over(v2):
    """d with v2 + d * d == the next float32 above v2 (d * d lies between half an ulp and one and a half)."""
    v2 = F(v2)
    d = F(np.sqrt(np.float64(np.nextafter(v2, F(np.inf))) - np.float64(v2)))
    assert v2 + d * d == np.nextafter(v2, F(np.inf))
    return d


def _scan(points):
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return p[:, 0].astype(F), p[:, 1].astype(F)


SEP = [(100.0, 50.0), (110.0, 50.0), (120.0, 50.0)]


def scenarios():
    """name -> (bx, by, keywords of detect(), expected dict(segments, accepted, ndet))."""
    s = {}

    def add(name, points, segments, accepted, ndet=None, **kw):
        bx, by = _scan(points)
        s[name] = (bx, by, dict(KW, **kw), dict(segments=segments, accepted=accepted, ndet=accepted if ndet is None else ndet))

    # 1. the jump: g == jump2 exactly does not break, the next float32 up does
    add("jump_equal", [SEP[0], (0, 0), (JUMP, 0), SEP[1]], 3, 1)
    add("jump_above", [SEP[0], (0, 0), (JUMP, just_over(JUMP * JUMP)), SEP[1]], 4, 0)
    # 2. the point count: clusters of 1, 2, 4 and 5 points (min_points - 1, min_points, max_points, max_points + 1)
    pts = []
    for k, m in enumerate((1, 2, 4, 5)):
        pts += [(10.0 * k + 0.1 * j, 5.0) for j in range(m)]
    add("point_counts", pts, 4, 2)
    # 3. the width: exactly width2, and one ulp over
    add("width_equal", [SEP[0], (0, 0), (0.25, 0), (WIDTH, 0), SEP[1]], 3, 1, max_points=8)
    add("width_above", [SEP[0], (0, 0), (0.25, 0), (WIDTH, just_over(WIDTH * WIDTH)), SEP[1]], 3, 0, max_points=8)
    # 4. occlusion.  Left: p = (0, 0) in front of f = (guard, 0): g_f == guard2 occludes, one ulp over does not, nor does r2_p == r2_f
    over = just_over(GUARD * GUARD)
    add("left_guard_equal", [SEP[0], (0, 0), (GUARD, 0), (1.1, 0), (1.2, 0), SEP[1]], 4, 0)
    add("left_guard_above", [SEP[0], (0, 0), (GUARD, over), (1.1, over), (1.2, over), SEP[1]], 4, 1)
    add("left_equal_range", [SEP[0], (-0.5, 0), (0.5, 0), (0.5, 0.1), (0.5, 0.2), SEP[1]], 4, 1)
    #    right: q = (0, 0) behind e = (-guard, 0)
    add("right_guard_equal", [SEP[0], (-1.2, 0), (-1.1, 0), (-GUARD, 0), (0, 0), SEP[1]], 4, 0)
    add("right_guard_above", [SEP[0], (-1.2, over), (-1.1, over), (-GUARD, over), (0, 0), SEP[1]], 4, 1)
    add("right_equal_range", [SEP[0], (-0.5, 0.2), (-0.5, 0.1), (-0.5, 0), (0.5, 0), SEP[1]], 4, 1)
    # 5. a segment through P - 1 into 0, and the same scan without wrap: both edge pieces go, the interior cluster stays
    c = [(0.1 * j, 5.0) for j in range(4)]
    inner = [(20.0 + 0.1 * j, 5.0) for j in range(3)]
    ring = [c[2], c[3], SEP[0]] + inner + [SEP[1], c[0], c[1]]
    add("wrap_segment", ring, 4, 2)
    add("wrap_segment_no_wrap", ring, 5, 1, wrap=0)
    # 6. a NaN point breaks, and so does its successor; its own segment is rejected (min_points = 1: the separators are detections)
    nan = float("nan")
    add("nan_point", [SEP[0], (0, 5), (0.1, 5), (nan, nan), (0.2, 5), (0.3, 5), SEP[1]], 5, 4, min_points=1)
    add("nan_x_only", [SEP[0], (0, 5), (0.1, 5), (nan, 5), (0.2, 5), (0.3, 5), SEP[1]], 5, 4, min_points=1)
    # 7. no points, one point
    add("empty", [], 0, 0)
    add("one_point_wrap", [(1.0, 2.0)], 0, 0, min_points=1)          # its gap to itself is 0: no break, no segment
    add("one_point_no_wrap", [(1.0, 2.0)], 1, 0, min_points=1, wrap=0)   # a break, but the segment holds point 0
    # 8. no break at all
    a = 2 * np.pi * np.arange(12) / 12
    add("no_break", np.stack([0.2 * np.cos(a), 0.2 * np.sin(a)], 1), 0, 0, max_points=64)
    # 9. exactly one break with wrap: the segment is the whole scan, p = e and q = f by the index rule
    add("one_break_symmetric", [(-0.225, 5), (-0.075, 5), (0.075, 5), (0.225, 5)], 1, 1)   # r2_e == r2_f: occluded at neither end
    add("one_break_skew", [(0.0, 5), (0.15, 5), (0.3, 5), (0.45, 5)], 1, 0)                # q = f is nearer than e: occluded
    # 10. more than 64 accepted segments: the first 64 by start index, the stats show the rest
    pts = []
    for k in range(70):
        pts += [(3.0 * k, 50.0), (3.0 * k + 0.1, 50.0)]
    add("many", pts, 70, 70, ndet=64)
    return s


def pole_field(P, seed, wrap_pole=True):
    """A random scan of P points: a round wall at about 0.1 m between neighbouring points, poles of 1 .. 7 points in front of it
    every 3 .. 24 points, some with a nearer pole right beside them (an occluder), one across the end of the scan.
    -> (bx, by, keywords of detect())."""
    rng = np.random.default_rng(seed)
    R = max(0.1 * P / (2 * np.pi), 0.5)
    r = R * (1 + 0.0005 * rng.standard_normal(P))
    b = int(rng.integers(0, 6))
    while b < P:
        m = int(rng.integers(1, 8))
        near = R * rng.uniform(0.4, 0.9)
        r[b:b + m] = near * (1 + 0.002 * rng.standard_normal(len(r[b:b + m])))
        b += m
        if rng.random() < 0.25:                    # a nearer pole right beside it
            m2 = int(rng.integers(1, 4))
            r[b:b + m2] = near - rng.uniform(0.2, 0.6)
            b += m2
        b += int(rng.integers(3, 25))
    if wrap_pole and P >= 32:
        r[[P - 2, P - 1, 0, 1]] = 0.7 * R
        r[[P - 4, P - 3, 2, 3]] = R
    a = -np.pi + 2 * np.pi * np.arange(P) / max(P, 1)
    kw = dict(D.DEFAULTS, max_range=1000.0, max_points=40)
    return (r * np.cos(a)).astype(F), (r * np.sin(a)).astype(F), kw
