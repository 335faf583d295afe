"""Hand-made scans, one per edge of the fitted detector's rule (tests/_detect_fit_spec.py).  TEST INFRASTRUCTURE shared by
test_detect_fit_spec_cpu.py (which checks what the specification makes of each) and test_gpu_detect_fit.py (which runs the kernel on
the same scans).  Like tests/_detect_scenes.py, whose separators and keywords these scans use: the critical points are dyadic
numbers about an axis, so that the centroid, the differences to it and their squares are exact and the spread s2 can be placed ON
the limit or one float32 above it."""
import numpy as np

import _detect_scenes as S

F = np.float32
H = F(0.125)            # half the distance of the critical pair: s2 = H * H exactly
X = F(5.0)


def _scan(points):
    p = np.asarray(points, np.float64).reshape(-1, 2)
    return p[:, 0].astype(F), p[:, 1].astype(F)


def pair(dy=0.0, x=X):
    """SEP, (x - H, -dy), (x + H, +dy), SEP: one segment of two points with centroid (x, 0) and s2 = H*H + dy*dy, all exact."""
    return _scan([S.SEP[0], (x - H, -dy), (x + H, dy), S.SEP[1]])


def scenarios():
    """name -> (bx, by, keywords of detect_fit(), fit, expected stats [segments, accepted, written, shape])."""
    s = {}
    over = S.just_over(H * H)
    # 1. the shape test: s2 == lim exactly is accepted (and rho2 - s2 == 0: the centroid itself), the next float32 up is not
    s["spread_equal"] = (*pair(), S.KW, (H, 0.0), [3, 1, 1, 0])
    s["spread_above"] = (*pair(over), S.KW, (H, 0.0), [3, 0, 0, 1])
    # ... and with a tolerance: s2 = H*H + (H/2)*(H/2) == lim = rho2 + tol2, every term exact (and rho2 - s2 < 0: clamped)
    s["spread_equal_tol"] = (*pair(0.0625), S.KW, (H, 0.0625), [3, 1, 1, 0])
    s["spread_above_tol"] = (*pair(0.0625), S.KW, (H, 0.03125), [3, 0, 0, 1])
    # 2. rho2 - s2 < 0 inside the tolerance: clamped to 0, the detection is the centroid
    s["clamped"] = (*pair(), S.KW, (0.0625, 0.125), [3, 1, 1, 0])
    # 3. an ordinary fit: the centre lies sqrt(rho2 - s2) behind the centroid
    s["behind"] = (*pair(), S.KW, (0.25, 0.0), [3, 1, 1, 0])
    # 4. a segment symmetric about the sensor: c2 == 0, no line of sight — counted with the shape rejections
    s["on_the_sensor"] = (*pair(x=F(0.0)), S.KW, (0.25, 0.0), [3, 0, 0, 1])
    # 5. the centroid (5 m out) within max_range, the fitted point (5.2165 m) beyond it: rejected, not by the shape test
    s["fitted_out_of_range"] = (*pair(), dict(S.KW, max_range=5.1), (0.25, 0.0), [3, 0, 0, 0])
    s["fitted_in_range"] = (*pair(), dict(S.KW, max_range=5.25), (0.25, 0.0), [3, 1, 1, 0])
    # 6. more than 64 accepted segments: the first 64 by start index
    bx, by, kw, _ = S.scenarios()["many"]
    s["many"] = (bx, by, kw, (0.1, 0.0), [70, 70, 64, 0])
    # 7. NaN and inf points: they break, their own segments pass no test, the neighbours are fitted
    nan, inf = float("nan"), float("inf")
    for name, bad in (("nan_point", (nan, nan)), ("inf_point", (inf, 5.0)), ("minus_inf_point", (5.0, -inf))):
        s[name] = (*_scan([S.SEP[0], (0, 5), (0.1, 5), bad, (0.2, 5), (0.3, 5), S.SEP[1]]), dict(S.KW, min_points=1), (0.1, 0.0),
                   [5, 4, 4, 0])
    return s


def arc_scene(lead, m=64, rho=0.1, centre=(2.0, 0.3), half_angle=80.0, roll=0):
    """`lead` separator points, an arc of m points of the circle (centre, rho) facing the sensor, two more separators; rolled by
    `roll` places (the arc through P - 1 into 0).  -> (bx, by, keywords with max_points = 64)."""
    c = np.asarray(centre, np.float64)
    back = np.arctan2(-c[1], -c[0])                      # from the centre towards the sensor
    phi = back + np.deg2rad(np.linspace(-half_angle, half_angle, m))
    arc = np.stack([c[0] + rho * np.cos(phi), c[1] + rho * np.sin(phi)], 1)
    pts = [(100.0 + 10.0 * j, 50.0) for j in range(lead)] + arc.tolist() + [(100.0, 80.0), (110.0, 80.0)]
    bx, by = _scan(pts)
    return np.roll(bx, roll), np.roll(by, roll), dict(S.KW, min_points=3, max_points=64)
