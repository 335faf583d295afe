"""The ordered hit sum of the four-lanes-per-pose scorer (csrc/score_body.h: add_hit): every lane of a quad adds the quad's
four hits in beam order, the quad broadcast folded into the addition.  The additions, their operands and their order are the
reference's sequential float sum; `score` and `count` are compared BIT FOR BIT with the CPU specification.

Stand-alone scorer (slam_score_poses_dev):
  3 073 poses: one above kWaveMaxPoses (3 072), where the quad form starts; 3 075: a last wavefront with unused quads;
  beams 1 and 3 (fewer than a quad), 33 (a padded second round of 32), 360 (the workload's count);
  on the float grid (a grid whose values are not in the packed code set stays a float grid at every pose count) and on the
  packed byte copy.
Fused front launch: n = 4 099, L = 261, the smallest shape tests/test_gpu_front_diet.py runs it at (its world and session, on
bench.py's room with one cell in 500 occupied at random: next to the room's straight walls alone the hits are small integers,
their sums are exact and no order of additions shows — 0 of 4 099 poses in a settled frame); split with survivor rows on and
off, and rows; the launch scores with four lanes per pose at that size.

So that none of it passes vacuously, a CPU assertion on the very scans and poses: the float32 sum of the specification's hits
in beam order differs in bits from the sum of the same hits in reversed order for a nonzero number of poses (reported).
PARITY UNPINNED for the fused front: the reference has no landmarks.
"""
import functools

import numpy as np
import pytest
import torch

import test_gpu_front_diet as D
import test_gpu_survivor_rows as S
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_frame_front_at_size import _tensor

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROWS, COLS, LD = 150, 190, 200
META = (ROWS, COLS, LD, 0.1, -3.0, -2.5)
NMAX = 3075


@functools.lru_cache(maxsize=None)
def _orc():
    import oracle

    oracle.build(ref=False)
    return oracle


def _hits(meta, edt, bx, by, x, y, th):
    """[pose][beam]: the hit of every beam by itself (a one-beam scan's score: 0 + h), +0 where the beam is out of bounds"""
    h = np.empty((len(x), len(bx)), np.float32)
    for b in range(len(bx)):
        h[:, b] = _orc().score_poses_det(meta, edt, bx[b:b + 1], by[b:b + 1], x, y, th)[0]
    return h


def _ordered_sum(h, order):
    t = np.zeros(h.shape[0], np.float32)
    for b in order:
        t = t + h[:, b]   # float32 + float32, one rounding per beam
    return t


def _order_matters(meta, edt, bx, by, x, y, th, want_score, what):
    h = _hits(meta, edt, bx, by, x, y, th)
    nb = len(bx)
    assert np.array_equal(bits(_ordered_sum(h, range(nb))), bits(want_score)), f"{what}: the hits do not add up to the specification's score"
    differ = int(np.count_nonzero(bits(_ordered_sum(h, range(nb - 1, -1, -1))) != bits(want_score)))
    print(f"{what}: {differ} of {len(x)} poses differ in bits between beam order and reversed order")
    return differ


@functools.lru_cache(maxsize=None)
def _room():
    """smoke()'s room: the packable EDT as the engine builds it, a float-only copy, 360 beams, 3 075 poses in the room's middle
    and along its left border (made once)"""
    rng = np.random.default_rng(7)
    occ = np.zeros((LD, LD), np.int32)
    occ[:ROWS, :COLS] = rng.random((ROWS, COLS)) < 0.02
    edt = _orc().edt(occ, ROWS, COLS, 10.0, "window")
    ang = np.linspace(-np.pi, np.pi, 360, endpoint=False)
    rad = rng.uniform(1.0, 6.0, 360)
    bx, by = (rad * np.cos(ang)).astype(np.float32), (rad * np.sin(ang)).astype(np.float32)
    x = (6.0 + 0.3 * rng.standard_normal(NMAX)).astype(np.float32)
    y = (5.0 + 0.3 * rng.standard_normal(NMAX)).astype(np.float32)
    th = (0.1 * rng.standard_normal(NMAX)).astype(np.float32)
    edge = np.arange(NMAX) % 8 == 5   # every eighth pose within 2 m of the grid's left border: some of its beams leave the grid
    x[edge] = (-3.0 + rng.uniform(0.0, 2.0, int(edge.sum()))).astype(np.float32)
    grids = {"packed": np.ascontiguousarray(edt, np.float32),
             "float": (edt * rng.uniform(0.9, 1.1, edt.shape)).astype(np.float32)}   # not sqrt of an integer: does not pack
    for g in grids.values():
        g.setflags(write=False)
    return grids, bx, by, x, y, th


@functools.lru_cache(maxsize=None)
def _want(grid, nbeams):
    """the specification's score and count of all 3 075 poses (a pose's score does not depend on the other poses)"""
    grids, bx, by, x, y, th = _room()
    return _orc().score_poses_det(_orc().meta(*META), grids[grid], bx[:nbeams], by[:nbeams], x, y, th)


@pytest.fixture(scope="module")
def eng():
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.mark.parametrize("nbeams", [1, 3, 33, 360])
@pytest.mark.parametrize("n", [3073, 3075])
@pytest.mark.parametrize("grid", ["float", "packed"])
def test_quad_scorer_against_the_cpu_specification(eng, grid, n, nbeams):
    grids, bx, by, x, y, th = _room()
    d_edt = torch.as_tensor(grids[grid].copy()).to(DEV)
    eng.grid_set_dev(1, d_edt, load_package().grid_meta(*META))
    eng.scan_upload(bx[:nbeams], by[:nbeams])
    dx, dy, dt = (torch.as_tensor(a[:n].copy()).to(DEV) for a in (x, y, th))
    sc = torch.full((n,), -1.0, device=DEV)
    cn = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    eng.score_poses_dev(1, dx, dy, dt, n, sc, cn)
    torch.cuda.synchronize()
    want_score, want_count = _want(grid, nbeams)
    assert np.array_equal(cn.cpu().numpy(), want_count[:n]), "in-bounds counts"
    assert nbeams < 33 or want_count.min() < want_count.max() == nbeams, "the in-bounds counts no longer vary"
    got = sc.cpu().numpy()
    bad = np.flatnonzero(bits(got) != bits(want_score[:n]))
    assert bad.size == 0, f"scores differ at {bad[:8]}: {got[bad[:8]]} != {want_score[bad[:8]]}"


@pytest.mark.parametrize("grid", ["float", "packed"])
def test_the_order_of_the_sum_shows_in_the_scorer_s_poses(grid):
    grids, bx, by, x, y, th = _room()
    differ = _order_matters(_orc().meta(*META), grids[grid], bx, by, x, y, th, _want(grid, 360)[0], f"{grid} grid, 360 beams")
    assert differ > 0, "the order of the sum does not show in any pose"


@functools.lru_cache(maxsize=None)
def _speckled_world(n):
    """test_gpu_front_diet's world with random occupied cells strewn over the room (made once; the shared world stays as it is)"""
    w = dict(D._world(n))
    pixel, min_x, min_y = w["meta"]
    occ = w["B"].occupancy(S.GRID, float(pixel), float(min_x), float(min_y)).copy()
    occ[np.random.default_rng(5).random(occ.shape) < 0.002] = 1
    eng = load_package().Engine(0)
    d_edt = torch.empty((S.GRID, S.GRID), dtype=torch.float32, device=S.DEV)
    eng.edt_dev(torch.from_numpy(occ).to(S.DEV), S.GRID, S.GRID, S.GRID, 10.0, d_edt)
    eng.sync()
    eng.close()
    w["d_edt"], w["edt"] = d_edt, d_edt.cpu().numpy()
    return w


@pytest.mark.parametrize("layout,survivor_rows", [("split", True), ("split", False), ("rows", False)])
def test_fused_front_scores_against_the_cpu_specification(orc, layout, survivor_rows):
    n, frames = 4099, 3
    w = _speckled_world(n)
    B = w["B"]
    ometa = orc.meta(*w["ometa_args"])
    eng, ses = D._session(w, n, layout, survivor_rows, -1)
    lanes, differ = set(), 0
    for f in range(frames):
        fr = w["fr"][f]
        v = ses.device_view()
        anc = None if v["anc"] is None else _tensor(v["anc"]).cpu().numpy()
        src_pose = _tensor(v["pose"]).cpu().numpy()
        fused_before = eng.frame_fusion_count()
        S._step(eng, ses, fr)
        eng.sync()
        assert eng.frame_fusion_count() - fused_before == (1 if f else 0), f"frame {f}: the front was not one fused launch"
        if f:
            lanes.add(eng.frame_front_last()[1])
        v = ses.device_view()
        x, y, th = orc.motion_sample(src_pose[0], src_pose[1], src_pose[2], anc, n, 0, fr["dp"], np.array(B.SIGMA, np.float32),
                                     S.SEED, f)
        assert np.array_equal(bits(_tensor(v["pose"]).cpu().numpy()), bits(np.stack([x, y, th]))), f"frame {f}: poses"
        want_score, want_count = orc.score_poses_det(ometa, w["edt"], fr["bx"], fr["by"], x, y, th)
        assert np.array_equal(_tensor(v["count"]).cpu().numpy()[:n], want_count), f"frame {f}: in-bounds counts"
        assert np.array_equal(bits(_tensor(v["score"]).cpu().numpy()[:n]), bits(want_score)), f"frame {f}: scores"
        if f:
            differ += _order_matters(ometa, w["edt"], fr["bx"], fr["by"], x, y, th, want_score, f"fused front {layout}, frame {f}")
    assert differ > 0, "the order of the sum does not show in any pose of any fused frame"
    assert lanes == {4}, lanes   # the lane mapping launch_frame_front chooses at this size
    S._close((eng, ses))
