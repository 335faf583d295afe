"""slam_pf_modes restated exactly (include/slam_hip.h): the heaviest clusters of a pose population on a grid of
cells (ix, iy, heading bin), from exact integer sums per cell.  numpy, Python integers and the oracle's deterministic functions;
nothing of the package under test.  TEST INFRASTRUCTURE."""
import math
from collections import namedtuple

import numpy as np

import oracle
from _estimate_spec import trunc_div, weights16  # noqa: F401  (weights16: what the tests make the 16-bit weights with)

F_SHIFT = 20                       # FX, FY, S, C: 2^-20 fixed point
F_ONE = np.float32(1048576.0)
U_LIMIT = np.float32(1048576.0)    # the domain: |x / cell|, |y / cell| < 2^20
INV_2PI = np.float32(0.15915494)
MAX_CELLS = 65536
MAX_MODES = 8

Mode = namedtuple("Mode", "pose mass cell ncells weight")
Result = namedtuple("Result", "modes cells wtotal")


class OutOfDomain(ValueError):
    """A particle lies outside |x / cell|, |y / cell| < 2^20 or has a coordinate that is not a number: SLAM_ERR_INVALID_ARG."""


class TooManyCells(ValueError):
    """More than MAX_CELLS distinct cells: SLAM_ERR_CAPACITY."""


def params_ok(cell, hbins, max_modes):
    c = np.float32(cell)
    return bool(np.isfinite(c) and c > 0) and (hbins == 1 or 4 <= hbins <= 64) and 1 <= max_modes <= MAX_MODES


def particle_terms(x, y, th, idx, ref_theta, cell, hbins, floor=np.floor):
    """-> (ix, iy, b, FX, FY, S, C) as int64 arrays, the particles behind the gather idx; raises OutOfDomain.
    `floor`: np.floor is the definition; np.trunc is what the kernel must NOT compute (negative coordinates tell them apart)."""
    x, y, th = (np.ascontiguousarray(a, np.float32) for a in (x, y, th))
    if idx is not None:
        idx = np.asarray(idx, np.int64)
        x, y, th = x[idx], y[idx], th[idx]
    inv = np.float32(1.0) / np.float32(cell)                      # once, on the host
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        ux, uy = (x * inv).astype(np.float32), (y * inv).astype(np.float32)
        if not (np.all(np.abs(ux) < U_LIMIT) and np.all(np.abs(uy) < U_LIMIT) and np.all(np.isfinite(th))):   # (a NaN is outside)
            raise OutOfDomain(int(np.count_nonzero(~((np.abs(ux) < U_LIMIT) & (np.abs(uy) < U_LIMIT) & np.isfinite(th)))))
        for u in (ux, uy):
            fl = floor(u).astype(np.float32)
            frac = (u - fl).astype(np.float32)                    # (exact but for u in (-2^-25, 0): 1.0f, so F = 2^20 in cell -1)
            out += [fl.astype(np.int64), (frac * F_ONE).astype(np.float32).astype(np.int64)]
        t = (th * INV_2PI).astype(np.float32)
        t = (t - np.floor(t)).astype(np.float32)
        b = np.minimum((t * np.float32(hbins)).astype(np.float32).astype(np.int64), hbins - 1)
    s, c = oracle.det_sincos((th - np.float32(ref_theta)).astype(np.float32))
    S = np.trunc(s.astype(np.float64) * 2.0 ** F_SHIFT).astype(np.int64)
    C = np.trunc(c.astype(np.float64) * 2.0 ** F_SHIFT).astype(np.int64)
    return out[0], out[2], b, out[1], out[3], S, C


def cell_table(x, y, th, idx, ref_theta, cell, hbins, w16=None, floor=np.floor):
    """-> {(ix, iy, b): [W, sum w FX, sum w FY, sum w S, sum w C]} in Python integers; raises OutOfDomain, TooManyCells.
    w16: one weight per SLOT (None, or all zero: w = 1); a particle of weight 0 makes no cell."""
    ix, iy, b, fx, fy, s, c = particle_terms(x, y, th, idx, ref_theta, cell, hbins, floor)
    w = [1] * len(ix) if w16 is None or not any(int(v) for v in w16) else [int(v) for v in w16]
    assert len(w) == len(ix)
    cells = {}
    for k, wi, *v in zip(zip(ix.tolist(), iy.tolist(), b.tolist()), w, fx.tolist(), fy.tolist(), s.tolist(), c.tolist()):
        if wi == 0:
            continue
        acc = cells.setdefault(k, [0, 0, 0, 0, 0])
        acc[0] += wi
        for j in range(4):
            acc[1 + j] += wi * v[j]
    if len(cells) > MAX_CELLS:
        raise TooManyCells(len(cells))
    return cells


def hdist(a, b, hbins):
    d = abs(a - b)
    return min(d, hbins - d)


def neighbours(key, hbins, reach=1):
    """the keys within `reach` cells of `key` in x and y and within `reach` bins, cyclically, in heading (each once)"""
    ix, iy, b = key
    bins = sorted({(b + d) % hbins for d in range(-reach, reach + 1)}) if hbins > 1 else [0]
    return [(ix + dx, iy + dy, bb) for dx in range(-reach, reach + 1) for dy in range(-reach, reach + 1) for bb in bins]


def select(cells, hbins, max_modes):
    """-> the centres, in order: the eligible cell of the largest score, the smallest key on ties"""
    score = {k: sum(cells[q][0] for q in neighbours(k, hbins) if q in cells) for k in cells}
    centres = []
    for _ in range(max_modes):
        best = None
        for k, sc in score.items():
            if any(abs(k[0] - c[0]) <= 2 and abs(k[1] - c[1]) <= 2 and hdist(k[2], c[2], hbins) <= 2 for c in centres):
                continue
            if best is None or sc > best[0] or (sc == best[0] and k < best[1]):
                best = (sc, k)
        if best is None:
            break
        centres.append(best[1])
    return centres


def mode_of(cells, centre, hbins, ref_theta, cell, wtotal):
    members = [q for q in neighbours(centre, hbins) if q in cells]
    wm = sum(cells[q][0] for q in members)
    pos = []
    for axis in (0, 1):
        a = sum(cells[q][0] * (q[axis] - centre[axis]) * (1 << F_SHIFT) + cells[q][1 + axis] for q in members)
        qd = trunc_div(a, wm)
        pos.append(np.float32((float(centre[axis]) + float(qd) / 1048576.0) * float(np.float32(cell))))
    ss, sc = (sum(cells[q][j] for q in members) for j in (3, 4))
    theta = np.float32(float(np.float32(ref_theta)) + math.atan2(float(ss), float(sc)))
    mass = np.float32(float(wm) / float(wtotal))
    return Mode(np.array([pos[0], pos[1], theta], np.float32), mass, tuple(centre), len(members), wm)


def modes_spec(x, y, th, idx, ref_theta, cell, hbins, max_modes, w16=None, floor=np.floor):
    """-> Result(modes, cells, wtotal); raises OutOfDomain (checked first) or TooManyCells."""
    assert params_ok(cell, hbins, max_modes)
    cells = cell_table(x, y, th, idx, ref_theta, cell, hbins, w16, floor)
    wtotal = sum(v[0] for v in cells.values())
    centres = select(cells, hbins, max_modes)
    return Result([mode_of(cells, c, hbins, ref_theta, cell, wtotal) for c in centres], len(cells), wtotal)


def same(a: Result, b: Result):
    """every field of every mode, the counts: bit for bit"""
    if (a.cells, a.wtotal, len(a.modes)) != (b.cells, b.wtotal, len(b.modes)):
        return False
    for p, q in zip(a.modes, b.modes):
        if not (np.array_equal(np.asarray(p.pose, np.float32).view(np.uint32), np.asarray(q.pose, np.float32).view(np.uint32))
                and np.float32(p.mass).view(np.uint32) == np.float32(q.mass).view(np.uint32)
                and tuple(int(v) for v in p.cell) == tuple(int(v) for v in q.cell) and int(p.ncells) == int(q.ncells)
                and int(p.weight) == int(q.weight)):
            return False
    return True


# ------------------------------------------------------------------ the pose populations the modes' tests add
def modes_population(name, n, cell=0.5, seed=0):
    """-> (x, y, th) float32 [n]"""
    rng = np.random.default_rng([seed, n, sum(map(ord, name))])
    c = float(cell)
    if name == "straddle_zero":      # a cluster centred on x = 0 (and y = 0): cells -1 and 0 under floor, all in 0 under the cast
        x = rng.normal(0.0, 0.02 * c, n).astype(np.float32)
        y = rng.normal(0.0, 0.02 * c, n).astype(np.float32)
        th = rng.normal(1.0, 0.01, n).astype(np.float32)
    elif name == "heading_wrap":     # headings on both sides of 0 / 2 pi: bins 0 and H - 1, one mode
        x = rng.normal(3.2 * c, 0.02 * c, n).astype(np.float32)
        y = rng.normal(-1.6 * c, 0.02 * c, n).astype(np.float32)
        th = (np.where(np.arange(n) % 2 == 0, 0.0, 2.0 * np.pi) + rng.normal(0.0, 0.05, n)).astype(np.float32)
    elif name == "scatter":          # uniform over 50 x 50 cells and all headings
        x = rng.uniform(-25.0 * c, 25.0 * c, n).astype(np.float32)
        y = rng.uniform(-25.0 * c, 25.0 * c, n).astype(np.float32)
        th = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    elif name in ("wave_64_keys", "wave_2_keys"):   # every run of 64 particles holds exactly 64 (2) distinct cells, the same in every run
        k = np.arange(n) % (64 if name == "wave_64_keys" else 2)
        x = ((k % 8) * 4 + 0.25 + 0.5 * rng.random(n)).astype(np.float32) * np.float32(c)
        y = ((k // 8) * 4 + 0.25 + 0.5 * rng.random(n)).astype(np.float32) * np.float32(c)
        th = rng.normal(1.0, 0.01, n).astype(np.float32)
    else:
        raise KeyError(name)
    return x, y, th


def two_blobs(n, gap_cells, cell=0.5, weight_ratio=1, seed=0):
    """two tight clusters in the middle of cells `gap_cells` cells apart in x, one heading; every (weight_ratio + 1)-th particle
    in the second (weight_ratio = 1: equal halves for even n)"""
    rng = np.random.default_rng([seed, n, gap_cells])
    c = float(cell)
    second = np.arange(n) % (weight_ratio + 1) == weight_ratio
    x = ((np.where(second, 10.5 + gap_cells, 10.5) + rng.uniform(-0.2, 0.2, n)) * c).astype(np.float32)
    y = ((7.5 + rng.uniform(-0.2, 0.2, n)) * c).astype(np.float32)
    th = rng.normal(1.0, 0.01, n).astype(np.float32)
    return x, y, th
