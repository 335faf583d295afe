"""The packed copy of a grid (csrc/score_kernels.hip: launch_edt_pack) and the bookkeeping that decides when it is made, reused
or thrown away (csrc/engine_match.hip: many_pose_grid): every cap, shape and change of grid.

The copy gives the same bits as the float grid, so a scorer that quietly stayed on the float grid — or on the copy of a grid that
has changed since — would pass every comparison of scores with the float grid it was meant to read ... or give plausible scores
of the previous map.  Every step here therefore asserts two things:

  (a) what the scorer returns equals, BIT FOR BIT, the CPU specification on the cells the grid holds NOW (score_poses_dev:
      oracle.score_poses_det; score_poses_cs_dev: oracle.score_pose per pose; motion_score_dev: oracle.motion_sample, then
      score_poses_det; refine_poses_dev: tests/_refine_spec.py);
  (b) slam_grid_packed_state equals what tests/_packed_spec.py says of those cells and of the calls since the grid changed
      (0 below 3 072 poses or under 8 rows / 16 columns, else 1 if the contents pack, 2 if not) — fixed on the CPU by
      tests/test_packed_spec_cpu.py.

3 072 poses run the four-lanes-per-pose form, 131 072 the one-lane form; 33 beams (a padded second round of 32).  The poses
are strewn over the grid and a margin around it: asserted for every set is that the in-bounds counts vary, reach all 33, and
that on each of the four sides some pose OUTSIDE the grid still has beams inside (beams cross that border).
Observed on the MI355X: cap 16.0 packs; the largest distance below the cap in a packed grid is sqrtf(250), as on the CPU.
PARITY UNPINNED: the reference has one lattice of 27 poses and no packed grid.
"""
import functools

import numpy as np
import pytest
import torch

import _packed_spec as PS
import _refine_spec as RS
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NB = 33
QUAD, LANE = 3072, 131072
ORIGIN = (-0.37, 0.21)


@functools.lru_cache(maxsize=None)
def _orc():
    import oracle

    oracle.build(ref=False)
    return oracle


def _geometry(shape, pixel=PS.PIXEL, origin=ORIGIN):
    rows, cols, ld = PS.shape_of(shape) if isinstance(shape, str) else shape
    return (rows, cols, ld, pixel, origin[0], origin[1])


@functools.lru_cache(maxsize=None)
def _scan(geo):
    """33 beams no longer than a third of the grid's short side, so that a pose in its middle keeps them all"""
    rows, cols, _, pixel = geo[:4]
    rng = np.random.default_rng(33)
    ang = np.linspace(-np.pi, np.pi, NB, endpoint=False)
    rad = rng.uniform(0.05, 0.35, NB) * min(rows, cols) * pixel
    bx, by = (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)
    for a in (bx, by):
        a.setflags(write=False)
    return bx, by


@functools.lru_cache(maxsize=None)
def _poses(geo, n, extra=0):
    """n (+ extra) poses over the grid and a margin of 0.3 short sides around it, any heading; made once and, with the
    specification's counts on an all-ones grid of that geometry, checked for what the module's docstring says of them"""
    rows, cols, ld, pixel, min_x, min_y = geo
    rng = np.random.default_rng(n + rows)
    m = 0.3 * min(rows, cols) * pixel
    x = rng.uniform(min_x - m, min_x + cols * pixel + m, n + extra).astype(np.float32)
    y = rng.uniform(min_y - m, min_y + rows * pixel + m, n + extra).astype(np.float32)
    th = rng.uniform(-np.pi, np.pi, n + extra).astype(np.float32)
    for a in (x, y, th):
        a.setflags(write=False)
    if not extra:
        bx, by = _scan(geo)
        _, cnt = _orc().score_poses_det(_orc().meta(*geo), np.ones((rows, ld), np.float32), bx, by, x, y, th)
        _assert_counts_vary(geo, x, y, cnt)
    return x, y, th


def _assert_counts_vary(geo, x, y, cnt):
    rows, cols, _, pixel, min_x, min_y = geo
    assert cnt.min() < cnt.max() == NB, "the in-bounds counts do not vary up to every beam"
    outside = {"left": x < min_x - pixel, "right": x > min_x + cols * pixel, "below": y < min_y - pixel, "above": y > min_y + rows * pixel}
    for side, sel in outside.items():
        assert np.any(cnt[sel] > 0), f"no pose beyond the grid's side '{side}' has a beam inside"


def dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # (a copy: the shared arrays are read-only)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def _same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype == np.float32:
        bad = np.flatnonzero(bits(got) != bits(want))
    else:
        bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[:6]}: {got[bad[:6]]} != {want[bad[:6]]}"


class Slot:
    """One grid slot of an engine with what the header lets its caller know: the cells it holds now, its geometry, and the
    largest scorer call since the cells last changed.  Every scorer call through it checks (a) and (b)."""

    def __init__(self, eng, slot):
        self.eng, self.slot = eng, slot
        self.cells = self.geo = None
        self.most = 0

    # ---- the ways a grid changes
    def upload(self, occ, geo, cap):
        """slam_grid_upload_host -> the EDT it returns, checked against the CPU oracle's"""
        rows, cols, ld = geo[:3]
        edt = self.eng.grid_upload(self.slot, occ, load_package().grid_meta(*geo), cap, want_edt=True)
        want = _orc().edt(occ, rows, cols, cap, "window")
        _same(edt[:rows, :cols].ravel(), want[:rows, :cols].ravel(), f"EDT at cap {cap}")
        self.holds(edt, geo)
        return edt

    def adopt(self, d_buf, geo):
        """slam_grid_set_dev of a device buffer; the cells are what the buffer holds at this moment"""
        self.eng.grid_set_dev(self.slot, d_buf, load_package().grid_meta(*geo))
        self.holds(host(d_buf), geo)

    def holds(self, cells, geo):
        self.cells, self.geo, self.most = np.ascontiguousarray(cells, np.float32), geo, 0

    def set_meta(self, geo):
        assert geo[:3] == self.geo[:3]
        self.eng.grid_set_meta(self.slot, load_package().grid_meta(*geo))
        self.geo = geo   # (the cells, and with them the verdict, stay)

    # ---- (b)
    def want_state(self):
        return PS.engine_state(self.cells, self.geo[0], self.geo[1], self.most)

    def check_state(self, what=""):
        got = self.eng.grid_packed_state(self.slot)
        assert got == self.want_state(), f"{what}: packed state {got}, the specification says {self.want_state()}"
        return got

    # ---- (a), one method per consumer
    def _begin(self, n):
        bx, by = _scan(self.geo)
        self.eng.scan_upload(bx, by)
        self.most = max(self.most, n)
        sc = torch.full((n,), -1.0, device=DEV)
        cn = torch.full((n,), -1, device=DEV, dtype=torch.int32)
        return _orc().meta(*self.geo), bx, by, sc, cn

    def score(self, n, what=""):
        m, bx, by, sc, cn = self._begin(n)
        x, y, th = _poses(self.geo, n)
        self.eng.score_poses_dev(self.slot, dev(x), dev(y), dev(th), n, sc, cn)
        want_s, want_c = _orc().score_poses_det(m, self.cells, bx, by, x, y, th)
        tag = f"{what} score_poses_dev n={n}"
        _same(host(cn), want_c, tag + " counts")
        _same(host(sc), want_s, tag + " scores")
        return self.check_state(tag)

    def score_cs(self, n, what=""):
        m, bx, by, sc, cn = self._begin(n)
        x, y, th = _poses(self.geo, n)
        ct, st = np.cos(th).astype(np.float32), np.sin(th).astype(np.float32)   # the caller's trig, whatever it is
        self.eng.score_poses_cs_dev(self.slot, dev(x), dev(y), dev(ct), dev(st), n, sc, cn)
        one = [_orc().score_pose(m, self.cells, bx, by, float(x[i]), float(y[i]), float(ct[i]), float(st[i]))[:2] for i in range(n)]
        tag = f"{what} score_poses_cs_dev n={n}"
        _same(host(cn), np.array([c for _, c in one], np.int32), tag + " counts")
        _same(host(sc), np.array([s for s, _ in one], np.float32), tag + " scores")
        return self.check_state(tag)

    def motion_score(self, n, with_anc, what=""):
        m, bx, by, sc, cn = self._begin(n)
        extra = 11 if with_anc else 0
        src = _poses(self.geo, n, extra) if extra else _poses(self.geo, n)
        anc = np.random.default_rng(n).integers(0, n + extra, n).astype(np.int32) if with_anc else None
        # (noise of a fifth of a cell: the poses stay strewn over the grid and its margin)
        dp, sig, seed, frame, first_id = [0.01, -0.005, 0.002], [0.02, 0.02, 0.004], 4242, 3, 1 << 33
        dst = tuple(torch.full((n,), -1.0, device=DEV) for _ in range(3))
        self.eng.motion_score_dev(self.slot, tuple(dev(a) for a in src), dev(anc) if with_anc else None, dst, n, first_id, dp, sig,
                                  seed, frame, sc, cn)
        x, y, th = _orc().motion_sample(src[0], src[1], src[2], anc, n, first_id, dp, sig, seed, frame)
        want_s, want_c = _orc().score_poses_det(m, self.cells, bx, by, x, y, th)
        _assert_counts_vary(self.geo, x, y, want_c)
        tag = f"{what} motion_score_dev n={n} anc={with_anc}"
        for got, want, name in zip(dst, (x, y, th), ("x", "y", "theta")):
            _same(host(got), want, f"{tag} {name}")
        _same(host(cn), want_c, tag + " counts")
        _same(host(sc), want_s, tag + " scores")
        return self.check_state(tag)

    def refine(self, n, what=""):
        m, bx, by, sc, cn = self._begin(n)
        x, y, th = _poses(self.geo, n)
        step_xy, step_theta = 0.05, 0.008727   # half a cell
        dx, dy, dt = dev(x), dev(y), dev(th)
        self.eng.refine_poses_dev(self.slot, dx, dy, dt, n, step_xy, step_theta, 1, sc, cn)
        want = RS.refine(_orc(), m, self.cells, bx, by, x, y, th, step_xy, step_theta, 1)
        tag = f"{what} refine_poses_dev n={n}"
        for got, exp, name in zip((dx, dy, dt, sc), want[:4], ("x", "y", "theta", "score")):
            _same(host(got), exp, f"{tag} {name}")
        _same(host(cn), want[4], tag + " counts")
        assert np.any(bits(want[0]) != bits(x)) or np.any(bits(want[1]) != bits(y)), "no pose moved: the case checks nothing"
        return self.check_state(tag)


def _buffer(cells):
    """a device buffer of the cells' size (padding columns included)"""
    return dev(np.ascontiguousarray(cells, np.float32))


# ------------------------------------------------------------------ caps
@pytest.mark.parametrize("case", sorted(PS.cap_cases()), ids=lambda c: f"{c[0]}-{c[1]}-cap{c[2]}")
def test_caps_through_grid_upload(eng, case):
    """every cap of tests/test_packed_spec_cpu.py, with its verdict from there"""
    shape, kind, cap = case
    packs = PS.cap_cases()[case]
    rows, cols, ld = PS.shape_of(shape)
    occ, cpu_edt = PS.edt_case(shape, kind, cap)
    s = Slot(eng, 1)
    edt = s.upload(occ, _geometry(shape), cap)
    assert s.check_state("fresh upload") == 0
    assert PS.packs(edt, rows, cols) == packs
    if kind == "sparse" and cap >= 15.9:   # the end of the code range is exercised, not assumed: on the engine's EDT
        assert PS.largest_root(edt, rows, cols) == PS.largest_root(cpu_edt, rows, cols) == 250
        print(f"cap {cap}: largest distance below the top value sqrtf({PS.largest_root(edt, rows, cols)}), top {PS.top_value(edt, rows, cols)}")
    if cap > 16 and kind == "dense":        # no cell reaches the cap: the 256th code stands for some sqrtf(k)
        assert PS.top_value(edt, rows, cols) < np.float32(cap)
    assert s.score(QUAD) == (1 if packs else 2)
    if shape == "23x37":
        assert s.score(LANE) == (1 if packs else 2)


# ------------------------------------------------------------------ shapes
@pytest.mark.parametrize("n", [QUAD, LANE])
@pytest.mark.parametrize("shape", sorted(PS.SHAPES) + sorted(PS.TOO_SMALL))
def test_shapes(eng, shape, n):
    """the grid the engine builds (packs) and its scaled copy (does not), uploaded and adopted; under 8 rows or 16 columns
    neither gets a verdict and both score right"""
    small = shape in PS.TOO_SMALL
    geo = _geometry(shape)
    occ, _ = PS.edt_case(shape, "sparse", 10.0)
    s = Slot(eng, 2)
    s.upload(occ, geo, 10.0)
    assert s.score(n, "uploaded") == (0 if small else 1)
    keep = _buffer(PS.scaled_case(shape, "sparse", 10.0))
    s.adopt(keep, geo)
    assert s.score(n, "scaled") == (0 if small else 2)


# ------------------------------------------------------------------ consumers
@pytest.mark.parametrize("grid", ["packs", "does not pack"])
def test_every_consumer(eng, grid):
    shape = "23x37"
    cells = PS.edt_case(shape, "sparse", 10.0)[1] if grid == "packs" else PS.scaled_case(shape, "sparse", 10.0)
    state = 1 if grid == "packs" else 2
    keep = _buffer(cells)
    s = Slot(eng, 3)
    calls = [lambda: s.score(QUAD), lambda: s.score_cs(QUAD), lambda: s.motion_score(QUAD, False), lambda: s.motion_score(QUAD, True),
             lambda: s.motion_score(LANE, False), lambda: s.motion_score(LANE, True), lambda: s.refine(QUAD), lambda: s.score(LANE)]
    for call in calls:   # each consumer as the FIRST many-pose call on a freshly adopted grid: it is the one that makes the copy
        s.adopt(keep, _geometry(shape))
        assert s.check_state("adopted") == 0
        assert call() == state
    for call in calls:   # ... and all of them on the copy the last one left
        assert call() == state


# ------------------------------------------------------------------ threshold
@pytest.mark.parametrize("grid", ["packs", "does not pack"])
def test_the_pose_count_that_asks_for_a_verdict(eng, grid):
    shape = "150x190"
    occ, edt = PS.edt_case(shape, "sparse", 10.0)
    s = Slot(eng, 0)
    if grid == "packs":
        s.upload(occ, _geometry(shape), 10.0)
    else:
        keep = _buffer(PS.scaled_case(shape, "sparse", 10.0))
        s.adopt(keep, _geometry(shape))
    state = 1 if grid == "packs" else 2
    assert s.score(QUAD - 1) == 0
    assert s.refine(QUAD - 1) == 0
    assert s.motion_score(QUAD - 1, True) == 0
    assert s.score(QUAD) == state
    assert s.score(100) == state     # a small call reads the float grid and leaves the verdict alone
    assert s.score(QUAD - 1) == state


# ------------------------------------------------------------------ changes of grid
def test_a_slot_grows_and_shrinks():
    """a fresh engine (no packed buffer yet): A, a larger B (the buffer is reallocated), a smaller C (it is reused: B's bytes lie
    behind C's), and A again under another cap"""
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    try:
        s = Slot(e, 1)
        for shape, kind, cap, state in (("23x37", "sparse", 10.0, 1), ("150x190", "dense", 17.0, 1), ("9x17", "sparse", 10.0, 1),
                                        ("150x190", "single", 17.0, 2), ("8x16", "sparse", 3.5, 1), ("257x16", "sparse", 16.0, 1),
                                        ("23x37", "sparse", 3.5, 1)):
            occ, _ = PS.edt_case(shape, kind, cap)
            s.upload(occ, _geometry(shape), cap)
            assert s.check_state(f"{shape} uploaded") == 0
            assert s.score(QUAD, f"{shape} {kind} cap {cap}") == state
            assert s.score(QUAD, f"{shape} {kind} cap {cap} again") == state
    finally:
        torch.cuda.synchronize()
        e.close()


def test_edt_dev_into_the_adopted_buffer_is_noticed_by_itself(eng):
    shape = "150x190"
    rows, cols, ld = PS.shape_of(shape)
    geo = _geometry(shape)
    occ_a, edt_a = PS.edt_case(shape, "sparse", 10.0)
    occ_b, edt_b = PS.edt_case(shape, "dense", 10.0)
    occ_c, edt_c = PS.edt_case(shape, "single", 17.0)
    buf = torch.full((rows, ld), -1.0, device=DEV)
    other = torch.full((rows, ld), -1.0, device=DEV)
    s = Slot(eng, 1)

    def rebuild(occ, cap, want, into):
        eng.edt_dev(dev(occ), ld, rows, cols, cap, into)
        _same(host(into)[:, :cols].ravel(), want[:, :cols].ravel(), "slam_edt_dev")

    rebuild(occ_a, 10.0, edt_a, buf)
    s.adopt(buf, geo)
    assert s.score(QUAD, "A") == 1
    rebuild(occ_b, 10.0, edt_b, buf)   # in place: no call names the slot
    s.holds(host(buf), geo)
    assert s.check_state("rebuilt in place") == 0
    assert np.any(bits(edt_a) != bits(edt_b))
    assert s.score(QUAD, "B") == 1     # ... and the score follows the new cells
    rebuild(occ_a, 10.0, edt_a, other)   # an unrelated buffer: the state stays
    assert s.check_state("edt_dev elsewhere") == 1
    assert s.score(LANE, "B still") == 1
    rebuild(occ_c, 17.0, edt_c, buf)   # a grid that does not pack, in place, and back
    s.holds(host(buf), geo)
    assert s.check_state("rebuilt in place, C") == 0
    assert s.score(QUAD, "C") == 2
    rebuild(occ_a, 10.0, edt_a, buf)
    s.holds(host(buf), geo)
    assert s.check_state("rebuilt in place, A") == 0
    assert s.score(QUAD, "A again") == 1


def test_cells_rewritten_in_place_and_adopted_again(eng):
    """packable -> scaled in place (torch) -> packable again; slam_grid_set_dev after every rewrite, as the header asks"""
    shape = "23x37"
    geo = _geometry(shape)
    _, edt = PS.edt_case(shape, "sparse", 15.96)
    buf = _buffer(edt)
    s = Slot(eng, 1)
    s.adopt(buf, geo)
    assert s.score(QUAD, "packable") == 1
    buf.mul_(dev(np.random.default_rng(4).uniform(0.9, 1.1, edt.shape).astype(np.float32)))
    s.adopt(buf, geo)
    assert not PS.packs(s.cells, *geo[:2]) and s.check_state("adopted again") == 0
    assert s.score(QUAD, "scaled") == 2
    assert s.score(LANE, "scaled") == 2
    buf.copy_(dev(edt))
    s.adopt(buf, geo)
    assert s.check_state("adopted a third time") == 0
    assert s.score(QUAD, "packable again") == 1


def test_grid_set_meta_keeps_the_copy(eng):
    shape = "150x190"
    occ, _ = PS.edt_case(shape, "sparse", 15.9)
    s = Slot(eng, 1)
    s.upload(occ, _geometry(shape), 15.9)
    assert s.score(QUAD, "first geometry") == 1
    s.set_meta(_geometry(shape, pixel=0.05, origin=(2.5, -1.25)))
    assert s.check_state("after set_meta") == 1
    assert s.score(QUAD, "second geometry") == 1   # the poses and beams are laid out for the new pixel and origin
    assert s.score(LANE, "second geometry") == 1


def test_two_slots(eng):
    """two slots on one buffer: slam_edt_dev into it resets both; a third slot with a grid of its own is not disturbed, nor
    does it disturb them"""
    shape = "23x37"
    rows, cols, ld = PS.shape_of(shape)
    geo = _geometry(shape)
    occ_a, edt_a = PS.edt_case(shape, "sparse", 10.0)
    occ_b, edt_b = PS.edt_case(shape, "dense", 10.0)
    buf = _buffer(edt_a)
    a, b, c = Slot(eng, 0), Slot(eng, 1), Slot(eng, 2)
    a.adopt(buf, geo)
    b.adopt(buf, _geometry(shape, origin=(1.0, 2.0)))
    occ_c, _ = PS.edt_case("9x17", "single", 17.0)
    c.upload(occ_c, _geometry("9x17"), 17.0)
    assert c.score(QUAD, "third slot") == 2
    assert a.score(QUAD, "first slot") == 1
    assert b.check_state("second slot, not scored yet") == 0
    assert b.score(QUAD, "second slot") == 1
    eng.edt_dev(dev(occ_b), ld, rows, cols, 10.0, buf)
    for s in (a, b):
        s.holds(host(buf), s.geo)
        assert s.check_state("shared buffer rebuilt") == 0
    assert c.check_state("third slot") == 2
    assert b.score(QUAD, "second slot, new cells") == 1
    assert a.check_state("first slot, not scored yet") == 0
    assert c.score(QUAD, "third slot") == 2
    assert a.score(LANE, "first slot, new cells") == 1
    c.upload(occ_c, _geometry("9x17"), 10.0)   # the third slot changes: the other two keep their copies
    assert a.check_state("first slot") == 1 and b.check_state("second slot") == 1
    assert a.score(QUAD, "first slot") == 1 and b.score(QUAD, "second slot") == 1
    assert c.score(QUAD, "third slot, cap 10") == 1


def test_errors(eng):
    import ctypes as C

    pkg = load_package()
    fresh = pkg.Engine(0)
    try:
        for slot, status in ((0, -4), (3, -4), (-1, -2), (4, -2)):   # nothing in the slot / no such slot
            with pytest.raises(pkg.SlamError) as ei:
                fresh.grid_packed_state(slot)
            assert ei.value.status == status
        occ, _ = PS.edt_case("8x16", "sparse", 10.0)
        fresh.grid_upload(0, occ, pkg.grid_meta(*_geometry("8x16")), 10.0)
        assert fresh.grid_packed_state(0) == 0
        assert fresh.lib.slam_grid_packed_state(fresh.h, 0, None) == -2
        assert fresh.lib.slam_grid_packed_state(None, 0, C.byref(C.c_int(0))) == -2
    finally:
        fresh.close()


# ------------------------------------------------------------------ session
def test_session_follows_a_grid_rebuilt_in_place():
    """slam_pf_step (4 096 particles, 129 landmarks: the fused front launch) on an adopted grid; after three frames the grid is
    rebuilt IN PLACE by slam_edt_dev from a changed occupancy.  Poses and log-weights of every later frame equal, bit for bit,
    those of a second run in which the changed grid lives in a fresh buffer adopted with slam_grid_set_dev.  The set-up is
    tests/test_gpu_front_combined.py's."""
    import test_gpu_front_combined as F

    pkg = load_package()
    w = F._world(4096, 129, 360)
    B, n, grid = w["B"], w["n"], F.GRID
    pixel, min_x, min_y = np.float32(20.48 / grid), np.float32(-4.24), np.float32(-10.24)
    occ_a = B.occupancy(grid, float(pixel), float(min_x), float(min_y))
    occ_b = occ_a.copy()
    occ_b[np.random.default_rng(8).random(occ_b.shape) < 0.002] = 1   # furniture all over the room
    d_occ = {"a": F._tensor(occ_a), "b": F._tensor(occ_b)}
    change_at, frames = 3, F.FRAMES

    def run(in_place):
        eng = pkg.Engine(0)
        buf = torch.empty((grid, grid), dtype=torch.float32, device=F.DEV)
        fresh = torch.empty((grid, grid), dtype=torch.float32, device=F.DEV)
        torch.cuda.synchronize()
        eng.edt_dev(d_occ["a"], grid, grid, grid, 10.0, buf)
        eng.grid_set_dev(0, buf, pkg.grid_meta(grid, grid, grid, pixel, min_x, min_y))
        ses = pkg.PfSession(eng, n, w["L"], sigma=B.SIGMA, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN, seed=F.SEED, map_layout="split",
                            resample_ess_frac=0.0)
        ses.set_poses(*w["poses"])
        ses.set_map_dev(w["m0"], 5 * w["LP"], w["LP"])
        eng.sync()
        out, states, fused = [], [], 0
        for f in range(frames):
            if f == change_at:
                if in_place:
                    eng.edt_dev(d_occ["b"], grid, grid, grid, 10.0, buf)
                else:
                    eng.edt_dev(d_occ["b"], grid, grid, grid, 10.0, fresh)
                    eng.grid_set_dev(0, fresh, pkg.grid_meta(grid, grid, grid, pixel, min_x, min_y))
                assert eng.grid_packed_state(0) == 0, "the changed grid still has its old verdict"
            fused += F._step(eng, ses, w, f)[0]
            states.append(eng.grid_packed_state(0))
            v = ses.device_view()
            out.append({k: F._tensor(v[k]).cpu().numpy().copy() for k in ("pose", "logw", "score")})
        cells = (buf if in_place else fresh).cpu().numpy()
        ses.close()
        eng.close()
        return out, states, fused, cells

    one, states1, fused1, cells1 = run(True)
    two, states2, fused2, cells2 = run(False)
    assert states1 == states2 == [1] * frames, (states1, states2)
    assert fused1 == fused2 == frames - 1, "the frames after the first were meant for the fused front launch"
    _same(cells1.ravel(), cells2.ravel(), "the two runs' grids")
    assert PS.packs(cells1, grid, grid)
    for f in range(frames):
        for k in one[f]:
            _same(one[f][k].ravel(), two[f][k].ravel(), f"frame {f}: {k}")
    # ... and the change shows: the first frame on the new grid scores differently from that frame on the old one
    eng, ses = F._session(w, "packed", True)
    for f in range(change_at + 1):
        F._step(eng, ses, w, f)
    old = F._tensor(ses.device_view()["score"]).cpu().numpy()[:n].copy()
    F._close((eng, ses))
    differ = int(np.count_nonzero(bits(old) != bits(one[change_at]["score"][:n])))
    print(f"frame {change_at}: {differ} of {n} scores differ between the old grid and the new one")
    assert differ > 0, "the changed occupancy does not show in any score: a stale copy would go unnoticed"
