"""The specification of scan-match refinement ("Refinement") in numpy, on top of the CPU oracle's
`score_poses_det`.  TEST INFRASTRUCTURE shared by test_refine_spec_cpu.py and the GPU tests.

One sweep around a pose (x, y, th) with steps t (metres, x AND y) and r (radians):
  candidates th_a = {th - r, th, th + r}, x_i = {x - t, x, x + t}, y_j = {y - t, y, y + t}, one float32 subtract or add each
  (oracle/slam_oracle.c:262-264), scored by score_poses_det; the centre is the incumbent; the 27 candidates are visited
  theta-major, x, y-minor and one replaces the incumbent only with a strictly lower score; the pose becomes the winner.
"""
import numpy as np


def make_room(orc, rows=200, cols=200, ld=None, pixel=0.1, wall=20, nbeams=360, cap=10.0):
    """A rectangle of walls `wall` cells inside a rows x cols grid centred on the origin, its capped EDT, and the scan a
    sensor at pose (0, 0, 0) sees of it (one return per beam, on the wall).  -> (meta, edt[rows][ld], bx, by)"""
    ld = cols if ld is None else ld
    occ = np.zeros((rows, ld), np.int32)
    occ[wall, wall:cols - wall] = occ[rows - 1 - wall, wall:cols - wall] = 1
    occ[wall:rows - wall, wall] = occ[wall:rows - wall, cols - 1 - wall] = 1
    min_x, min_y = -pixel * cols / 2, -pixel * rows / 2
    edt = orc.edt(occ, rows, cols, cap, "window")
    meta = orc.meta(rows, cols, ld, pixel, min_x, min_y)
    # wall planes in metres (cell c covers the points that round to c: its centre is min + c * pixel)
    x0, x1 = min_x + wall * pixel, min_x + (cols - 1 - wall) * pixel
    y0, y1 = min_y + wall * pixel, min_y + (rows - 1 - wall) * pixel
    ang = np.linspace(-np.pi, np.pi, nbeams, endpoint=False) + 0.0123
    c, s = np.cos(ang), np.sin(ang)
    with np.errstate(divide="ignore"):
        d = np.minimum(np.where(c > 0, x1 / c, x0 / c), np.where(s > 0, y1 / s, y0 / s))
    return meta, edt, (d * c).astype(np.float32), (d * s).astype(np.float32)


def sweep(orc, meta, edt, bx, by, x, y, th, step_xy, step_theta):
    """One sweep for n poses -> (x, y, th, score, count, winner index 0..26 (13: the centre stayed))"""
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    n = len(x)
    t, r = np.float32(step_xy), np.float32(step_theta)
    ths, xs, ys = [th - r, th, th + r], [x - t, x, x + t], [y - t, y, y + t]
    cx = np.stack([xs[i] for a in range(3) for i in range(3) for j in range(3)]).astype(np.float32)
    cy = np.stack([ys[j] for a in range(3) for i in range(3) for j in range(3)]).astype(np.float32)
    ct = np.stack([ths[a] for a in range(3) for i in range(3) for j in range(3)]).astype(np.float32)
    sc, cn = orc.score_poses_det(meta, edt, bx, by, cx.ravel(), cy.ravel(), ct.ravel())
    sc, cn = sc.reshape(27, n), cn.reshape(27, n)
    best, win = sc[13].copy(), np.full(n, 13)
    for c in range(27):
        better = sc[c] < best
        best[better] = sc[c][better]
        win[better] = c
    k = np.arange(n)
    return cx[win, k], cy[win, k], ct[win, k], best, cn[win, k].astype(np.int32), win


def refine(orc, meta, edt, bx, by, x, y, th, step_xy, step_theta, sweeps, history=None):
    """`sweeps` sweeps, each re-centred on the winner -> (x, y, th, score, count); history (a list) receives every sweep's
    (x, y, th, score, count, win)."""
    assert 1 <= sweeps <= 16
    out = None
    for _ in range(sweeps):
        out = sweep(orc, meta, edt, bx, by, x, y, th, step_xy, step_theta)
        x, y, th = out[0], out[1], out[2]
        if history is not None:
            history.append(out)
    return out[:5]
