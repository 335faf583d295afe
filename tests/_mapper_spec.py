"""The mapper's frame loop written with the oracle's STAGE functions, and the generated cases both mapper test files share.

``MapperSpec`` mirrors ``orc_slam_first_frame`` / ``orc_slam_next_frame`` (oracle/slam_oracle.c) line by line, but calls
``oracle.clean_scan``, ``transform``, ``local_map``, ``rasterise``, ``edt(variant="window")`` and ``fastmatch`` one at a time
and keeps what each of them produced, so that a test can compare every intermediate of a frame with the device's —
``orc_slam_*`` itself only shows the pose and the map.  tests/test_mapper_spec_cpu.py pins this class to ``orc_slam_*``.

The cases are generated: a numpy ray-caster for a rectangular room (optionally with box obstacles) seen from a given pose
gives the ranges, so that a test controls them exactly; ``put`` overwrites chosen beams.
"""
from __future__ import annotations

import numpy as np

MAP_CAP = 20000 + 4096   # orc_slam_next_frame's clamp (slam_oracle.c); the engine's is 20000 + nbeams
LD = (200, 400)          # main.c:201, :207


class MapperSpec:
    def __init__(self, orc, nbeams, angle_min, angle_inc, params=None):
        self.o = orc
        self.nbeams = nbeams
        self.par = params if params is not None else orc.SlamParams.default()
        self.angles = orc.beam_angles(angle_min, angle_inc, nbeams)   # main.c:845
        z = lambda n: np.zeros(n, np.float32)
        self.sx, self.sy = z(0), z(0)         # cleaned scan [0, scan_n)
        self.tx, self.ty = z(0), z(0)         # world points, as long as the scan that made them
        self.map_x, self.map_y = z(0), z(0)
        self.lx, self.ly = z(0), z(0)
        self.occ = [np.zeros((ld, ld), np.int32) for ld in LD]
        self.edt = [np.zeros((ld, ld), np.float32) for ld in LD]
        self.meta = [orc.meta(0, 0, ld, 1.0, 0.0, 0.0) for ld in LD]
        self.hits = z(max(nbeams, 1))         # the persistent scratch: lives as long as the mapper
        self.hits_n = 0
        self.pose, self.prev, self.map_pose = z(3), z(3), z(3)
        self.mini_updated, self.frame = 1, 0
        # what the last frame did
        self.made_world = self.rebuilt = self.key = self.partial = False
        self.map_before = 0
        self.candidates = self.appended = 0
        self.crop_keep = None

    @property
    def scan_n(self):
        return len(self.sx)

    @property
    def map_n(self):
        return len(self.map_x)

    def _clean(self, ranges):
        p = self.par
        self.sx, self.sy = self.o.clean_scan(ranges, self.angles, p.range_min, p.usable_range)

    def _to_world(self, pose):
        self.tx, self.ty = self.o.transform(self.sx, self.sy, pose)
        self.made_world = True

    def first_frame(self, ranges):
        # orc_slam_first_frame: scan 0 at the origin seeds the map; the loop starts "mini-updated"
        self.made_world = self.rebuilt = self.key = self.partial = False
        self._clean(ranges)
        self._to_world(np.zeros(3, np.float32))
        self.map_before = 0
        self.map_x, self.map_y = self.tx.copy(), self.ty.copy()
        self.map_pose[:] = 0
        self.pose[:] = 0
        self.prev[:] = 0
        self.mini_updated, self.frame = 1, 1

    def _build_grids(self):
        o, p = self.o, self.par
        self.lx, self.ly = o.local_map(self.map_x, self.map_y, self.tx, self.ty, p.border)
        # the same crop in numpy, as a mask over the map (for the cases' conditions; checked against local_map by the CPU test)
        b = np.float32(p.border)
        lo_x, hi_x = self.tx.min() - b, self.tx.max() + b
        lo_y, hi_y = self.ty.min() - b, self.ty.max() + b
        self.crop_keep = (self.map_x > lo_x) & (self.map_x < hi_x) & (self.map_y > lo_y) & (self.map_y < hi_y)
        for k, pix in enumerate((p.pixel, p.pixel2)):
            self.occ[k], self.meta[k] = o.rasterise(self.lx, self.ly, pix, LD[k])
        for k in (0, 1):
            m = self.meta[k]
            assert 1 <= m.rows <= LD[k] and 1 <= m.cols <= LD[k], "the reference overruns its grid here (SURVEY Q8)"
            o.edt(self.occ[k], m.rows, m.cols, p.edt_cap, "window", out=self.edt[k])   # cells outside keep their content (Q7)
        self.rebuilt = True

    def _match(self, which, pose, res):
        out, _, self.hits_n, _ = self.o.fastmatch(self.meta[which], self.edt[which], self.sx, self.sy, pose, res, self.hits,
                                                  self.hits_n)
        return out

    def next_frame(self, ranges):
        p = self.par
        self.made_world = self.rebuilt = self.key = False
        self.candidates = self.appended = 0
        self.map_before = self.map_n
        self._clean(ranges)   # main.c:863
        if self.mini_updated:   # main.c:865-872: world points from the OLD pose (Q3)
            self._to_world(self.pose)
            self._build_grids()
        # main.c:875-898: constant-velocity guess, no angle wrapping
        guess = self.pose + (self.pose - self.prev) if self.frame > 1 else self.pose.copy()
        # main.c:901-918: the coarse step runs on the fine grid when the map was not just rebuilt (Q4)
        m1 = self._match(0 if self.mini_updated else 1, guess, np.array(list(p.fast_res), np.float32))
        m2 = self._match(1, m1, np.array(list(p.fast_res2), np.float32))
        self.prev = self.pose.copy()
        self.pose = m2.copy()
        self.partial = self.hits_n < self.scan_n
        # main.c:928-961
        d = np.abs(self.pose - self.map_pose)
        if d[0] > np.float32(p.key_dt) or d[1] > np.float32(p.key_dt) or d[2] > np.float32(p.key_dr):
            self.key = True
            self.mini_updated = 1
            if not self.made_world:
                self._to_world(self.pose)
            # hits of the LAST candidate, count of the BEST one, world points by in-bounds ordinal (Q2)
            cand = np.nonzero(self.hits[: self.hits_n] > np.float32(p.new_point_threshold))[0]
            take = cand[: max(MAP_CAP - self.map_n, 0)]
            self.candidates, self.appended = len(cand), len(take)
            self.map_x = np.concatenate([self.map_x, self.tx[take]])
            self.map_y = np.concatenate([self.map_y, self.ty[take]])
            self.map_pose = self.pose.copy()
        else:
            self.mini_updated = 0
        self.frame += 1
        return self.pose.copy()


# ------------------------------------------------------------------ the case generator


def cast(room, pose, angles, boxes=()):
    """Ranges (float32) of beams at sensor-frame `angles` from `pose` = (x, y, theta) inside the axis-aligned `room`
    = (x0, x1, y0, y1), stopped by the nearest of its walls and of the axis-aligned `boxes` (same 4-tuples).  A beam at
    sensor angle a points along world angle a - theta: the reference's world transform is the transposed rotation."""
    px, py, th = (float(v) for v in pose)
    a = np.asarray(angles, np.float64) - th
    dx, dy = np.cos(a), np.sin(a)
    with np.errstate(divide="ignore", invalid="ignore"):
        x0, x1, y0, y1 = room
        t = np.minimum(np.where(dx > 0, (x1 - px) / dx, np.where(dx < 0, (x0 - px) / dx, np.inf)),
                       np.where(dy > 0, (y1 - py) / dy, np.where(dy < 0, (y0 - py) / dy, np.inf)))
        for bx0, bx1, by0, by1 in boxes:
            tx0, tx1 = (bx0 - px) / dx, (bx1 - px) / dx
            ty0, ty1 = (by0 - py) / dy, (by1 - py) / dy
            enter = np.maximum(np.minimum(tx0, tx1), np.minimum(ty0, ty1))
            leave = np.minimum(np.maximum(tx0, tx1), np.maximum(ty0, ty1))
            t = np.where((enter <= leave) & (enter > 0), np.minimum(t, enter), t)
    return t.astype(np.float32)


def put(ranges, beams, values):
    """A copy of `ranges` with the chosen beams overwritten."""
    r = np.array(ranges, np.float32)
    r[np.asarray(beams, np.int64)] = np.asarray(values, np.float32)
    return r


def keep_only(ranges, keep):
    """A copy of `ranges` whose beams outside the boolean mask `keep` read 0 (below range_min: the clean-up drops them)."""
    return np.where(keep, ranges, np.float32(0)).astype(np.float32)


class Case:
    def __init__(self, name, nbeams, frames, params=None, angle_min=None, angle_inc=None, **extra):
        self.name, self.nbeams, self.frames = name, nbeams, frames
        self.changes = params or {}
        self.angle_min = -np.pi if angle_min is None else angle_min
        self.angle_inc = 2 * np.pi / nbeams if angle_inc is None else angle_inc
        self.extra = extra
        assert all(f.shape == (nbeams,) and f.dtype == np.float32 for f in frames)

    def angles(self, orc):
        return orc.beam_angles(self.angle_min, self.angle_inc, self.nbeams)

    def orc_params(self, orc):
        return orc.SlamParams.default(**self.changes)

    def pkg_params(self, pkg):
        p = pkg.MapperParams.default()
        for k, v in self.changes.items():
            setattr(p, k, type(getattr(p, k))(*v) if k in ("fast_res", "fast_res2") else v)
        return p

    def spec(self, orc):
        return MapperSpec(orc, self.nbeams, self.angle_min, self.angle_inc, self.orc_params(orc))


ROOM = (-4.0, 4.0, -3.0, 3.0)
BEAM_COUNTS = (1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096)


def survivor_patterns(n):
    """name -> boolean mask over n beams, for the patterns that exist at n."""
    k = np.arange(n)
    pat = {"all": k >= 0, "alternate": k % 2 == 0, "first": k == 0, "last": k == n - 1}
    if n >= 192:
        pat["wave_gap"] = (k < 64) | ((k >= 128) & (k < 192))   # one whole wavefront empty between two full ones
    if n > 1024:
        pat["batch1"] = k >= 1024                               # all of batch 0 dropped, all of batch 1 kept
    return pat


BEAM_CASES = [f"beams-{n}-{p}" for n in BEAM_COUNTS for p in survivor_patterns(n)]
CROP_SIZES = (1023, 1024, 1025, 2049)
OTHER_CASES = (["gate"] + [f"crop-size-{s}" for s in CROP_SIZES] +
               ["crop-border0", "crop-moved", "raster-200", "empty-frame", "append-grow", "append-threshold", "append-cap",
                "partial", "restart"])
ALL_CASES = BEAM_CASES + OTHER_CASES

GATE_BEAMS = (62, 63, 64, 65, 127, 128, 129, 130)


def gate_values(par):
    """(value, kept by the reference) for the gated beams, in GATE_BEAMS order."""
    lo, hi = np.float32(par.range_min), np.float32(par.usable_range)
    inf = np.float32(np.inf)
    return [(lo, True), (np.nextafter(lo, -inf), False), (np.nextafter(lo, inf), True), (hi, True),
            (np.nextafter(hi, -inf), True), (np.nextafter(hi, inf), False), (np.float32(0), False), (inf, False)]


# The growing room: every wall moves outward by 0.3 m a frame.  A grid has three cells of padding around its points and a beam
# must land inside it to count at all, so the fine cell is made one step wide (the new wall is ONE cell out, well inside the
# padding) and a new point is one more than half a cell from the map.
GROW = {"key_dt": 0.0, "key_dr": 0.0, "pixel": 0.6, "pixel2": 0.3, "new_point_threshold": 0.5}


def _grown(step, k):
    return (ROOM[0] - step * k, ROOM[1] + step * k, ROOM[2] - step * k, ROOM[3] + step * k)


def raster_room(orc, cols, nbeams=720):
    """A room whose first scan, cropped and rasterised as frame 1 does it, gives a coarse grid of exactly `cols` columns."""
    ang = orc.beam_angles(-np.pi, 2 * np.pi / nbeams, nbeams)
    for w in np.arange(38.0, 40.0, 0.01):
        room = (-w / 2, w / 2, -3.0, 3.0)
        x, y = orc.clean_scan(cast(room, (0, 0, 0), ang), ang)
        tx, ty = orc.transform(x, y, [0, 0, 0])
        lx, ly = orc.local_map(tx, ty, tx, ty, 1.0)
        # the column count alone, without the raster (201 columns do not fit the storage): main.c:297-305
        pix = np.float32(0.2)
        lo, hi = lx.min() - np.float32(3) * pix, lx.max() + np.float32(3) * pix
        n = int(np.floor(np.float64((hi - lo) / pix) + 0.5)) + 1
        if n == cols:
            return room
    raise AssertionError(f"no room gives {cols} columns")


_CASES = {}


def case(orc, name):
    if name not in _CASES:
        _CASES[name] = _make(orc, name)
    return _CASES[name]


def _make(orc, name):
    def angles(n):
        return orc.beam_angles(-np.pi, 2 * np.pi / n, n)

    if name.startswith("beams-"):
        _, n, pat = name.split("-")
        n = int(n)
        r = keep_only(cast(ROOM, (0.3, -0.2, 0), angles(n)), survivor_patterns(n)[pat])
        return Case(name, n, [r] * 4)
    if name == "gate":
        n = 360
        par = orc.SlamParams.default()
        r = put(cast(ROOM, (0, 0, 0), angles(n)), GATE_BEAMS, [v for v, _ in gate_values(par)])
        return Case(name, n, [r] * 3)
    if name.startswith("crop-size-"):
        n, s = 2049, int(name.rsplit("-", 1)[1])
        keep = np.zeros(n, bool)
        keep[np.round(np.linspace(0, n - 1, s)).astype(int)] = True
        assert keep.sum() == s
        r = keep_only(cast(ROOM, (0.2, 0.1, 0), angles(n)), keep)
        return Case(name, n, [r] * 3)
    if name == "crop-border0":
        n = 1500
        return Case(name, n, [cast(ROOM, (0, 0, 0), angles(n))] * 3, params={"border": 0.0})
    if name == "crop-moved":
        # a range limit below the room's half-diagonal: the sensor sees stretches of the walls only, and the stretches move with it
        n = 2049
        room = (-3.0, 3.0, -3.0, 3.0)
        boxes = [(1.0, 1.6, 2.4, 3.0), (-2.2, -1.6, -3.0, -2.5)]
        fr = [cast(room, (0.25 * k, 0.0, 0.0), angles(n), boxes) for k in range(8)]
        return Case(name, n, fr, params={"usable_range": 3.5, "border": 0.1, "key_dt": 0.3})
    if name in ("raster-200", "raster-201"):
        n = 720
        room = raster_room(orc, int(name[-3:]), n)
        return Case(name, n, [cast(room, (0, 0, 0), angles(n))] * 3)
    if name == "empty-frame":
        n = 360
        r = cast(ROOM, (0, 0, 0), angles(n))
        return Case(name, n, [r, r, np.zeros(n, np.float32), r, r])
    if name == "append-grow":
        n = 2049
        sizes = [0, 1, 2, 3, 3, 3]
        return Case(name, n, [cast(_grown(0.3, k), (0, 0, 0), angles(n)) for k in sizes], params=GROW)
    if name == "append-threshold":
        n = 720
        sizes = [0, 1, 2, 3, 4, 5]
        return Case(name, n, [cast(_grown(0.2, k), (0, 0, 0), angles(n)) for k in sizes],
                    params={"key_dt": 0.0, "key_dr": 0.0, "new_point_threshold": 2.0})
    if name == "append-cap":
        n = 4096
        sizes = list(range(8))
        return Case(name, n, [cast(_grown(0.3, k), (0, 0, 0), angles(n)) for k in sizes], params=GROW)
    if name == "partial":
        n = 720
        room = (-3.0, 30.0, -2.0, 2.0)
        boxes = [(2.0 + 3.0 * i, 2.6 + 3.0 * i, (1.4 if i % 2 else -2.0), (2.0 if i % 2 else -1.4)) for i in range(9)]
        fr = [cast(room, (0.25 * k, 0.0, 0.0), angles(n), boxes) for k in range(11)]
        return Case(name, n, fr, params={"key_dt": 0.6, "usable_range": 6.0})
    if name == "restart":
        n = 360
        boxes = [(2.0, 2.5, 1.0, 1.6)]
        fr = [cast(ROOM, (0.12 * k, 0.05 * k, 0.01 * k), angles(n), boxes) for k in range(5)]
        return Case(name, n, fr)
    raise KeyError(name)
