"""GPU parity of scan-match refinement (slam_refine_poses_dev, slam_motion_refine_dev) against its specification
(tests/_refine_spec.py on the CPU oracle): pose, score and count BIT FOR BIT in every case.

PARITY UNPINNED with respect to the reference: FastMatch runs its lattice around one pose, with libm trig and a start from
+inf; the refinement runs it around every pose with the particle path's trig and the centre as incumbent.

The launcher has ONE kernel form (three lanes per pose) in two grid flavours: the float grid below 3 072 poses
(kWaveMaxPoses: where the engine starts handing out the packed copy) or when the grid does not pack, the packed byte grid
otherwise.  It does not switch form at a larger pose count, so there is no further boundary to cross.  The pipeline round is
2 beams (one float2 pair).
"""
import numpy as np
import pytest
import torch

import _refine_spec as RS
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COARSE, FINE = (0.05, 0.008727), (0.025, 0.004363)


@pytest.fixture(scope="module")
def eng():
    pkg = load_package()
    e = pkg.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


class World:
    """A grid on the engine (slot 1) with its host copy, kept alive for the module."""

    def __init__(self, eng, meta, edt):
        pkg = load_package()
        self.meta, self.edt = meta, np.ascontiguousarray(edt, np.float32)
        self.keep = dev(self.edt)
        self.gm = pkg.grid_meta(meta.rows, meta.cols, meta.ld, meta.pixel, meta.min_x, meta.min_y)

    def bind(self, eng):
        eng.grid_set_dev(1, self.keep, self.gm)


def check(eng, orc, w, bx, by, x, y, th, steps, sweeps):
    """slam_refine_poses_dev against the specification; -> the specification's result"""
    w.bind(eng)
    eng.scan_upload(bx, by)
    n = len(x)
    dx, dy, dt = dev(x), dev(y), dev(th)
    sc = torch.full((n,), -1.0, device=DEV)
    cn = torch.full((n,), -1, device=DEV, dtype=torch.int32)
    eng.refine_poses_dev(1, dx, dy, dt, n, steps[0], steps[1], sweeps, sc, cn)
    want = RS.refine(orc, w.meta, w.edt, bx, by, x, y, th, steps[0], steps[1], sweeps)
    tag = f"n={n} beams={len(bx)} steps={steps} sweeps={sweeps}"
    for got, exp, name in zip((dx, dy, dt, sc), want[:4], "x y theta score".split()):
        g = host(got)
        bad = np.flatnonzero(bits(g) != bits(exp))
        assert bad.size == 0, f"{tag}: {name} differs at {bad[:8]}: {g[bad[:8]]} != {exp[bad[:8]]}"
    assert np.array_equal(host(cn), want[4]), tag
    return want


@pytest.fixture(scope="module")
def room(eng, orc):
    """the synthetic room of the CPU tests, ld != cols"""
    meta, edt, bx, by = RS.make_room(orc, rows=200, cols=190, ld=213)
    return World(eng, meta, edt), bx, by


@pytest.fixture(scope="module")
def state(eng, golden):
    """the golden state grids (coarse and fine) with the golden scan"""
    out = []
    for which in (0, 1):
        rows, cols, ld = (int(v) for v in golden[f"state_meta_{which}"])
        pix, minx, miny = (float(v) for v in golden[f"state_metaf_{which}"])
        import oracle
        edt = np.zeros((rows, ld), np.float32)
        edt[:, :cols] = golden[f"state_edt_{which}"]
        out.append(World(eng, oracle.meta(rows, cols, ld, pix, minx, miny), edt))
    return out, golden["scan_x_41"], golden["scan_y_41"]


def poses_around(rng, n, centre, spread=(0.15, 0.15, 0.03)):
    return tuple((np.float32(centre[k]) + spread[k] * rng.standard_normal(n)).astype(np.float32) for k in range(3))


@pytest.mark.parametrize("n", [1, 3, 64, 257, 3071, 3072, 3073])
def test_pose_counts_on_the_golden_grids(eng, orc, state, golden, n):
    """1 .. 257: a partly filled wavefront, one, several workgroups (84 poses each); 3 071 / 3 072 / 3 073: the float grid's
    last count and the packed grid's first two.  Poses around the golden lattice guesses, so that they sit in the map."""
    worlds, bx, by = state
    rng = np.random.default_rng(n)
    guess = golden["fm_guess"]
    for which in (0, 1):
        c = guess[rng.integers(0, len(guess), n)]
        x, y, th = (c[:, k] + s * rng.standard_normal(n) for k, s in enumerate((0.1, 0.1, 0.02)))
        out = check(eng, orc, worlds[which], bx, by, x.astype(np.float32), y.astype(np.float32), th.astype(np.float32), COARSE, 2)
        if n >= 64:
            assert np.any(bits(out[0]) != bits(x.astype(np.float32))), "no pose moved: the case checks nothing"


@pytest.mark.parametrize("nbeams", [0, 1, 2, 3, 7, 360, 1079])
@pytest.mark.parametrize("n", [100, 3100])
def test_beam_counts(eng, orc, room, nbeams, n):
    """0, 1 (one below the round of 2), 2 (a round), 3 (one above), 7, 360, 1 079 beams on the float grid (100 poses) and
    the packed one (3 100)."""
    w, _, _ = room
    _, _, bx, by = RS.make_room(orc, rows=200, cols=190, ld=213, nbeams=max(nbeams, 1))
    rng = np.random.default_rng(nbeams + n)
    x, y, th = poses_around(rng, n, (0, 0, 0))
    check(eng, orc, w, bx[:nbeams], by[:nbeams], x, y, th, COARSE, 2)


@pytest.mark.parametrize("sweeps", [1, 2, 5])
@pytest.mark.parametrize("steps", [COARSE, FINE, (0.0, 0.0), (100.0, 0.5)])
def test_sweeps_and_steps(eng, orc, room, sweeps, steps):
    """... including no step at all (pose, score and count of the scorer come back) and a step larger than the grid (every
    moved candidate is off the grid and scores 0 with count 0: the raw sum lets it win, as the specification says)."""
    w, bx, by = room
    rng = np.random.default_rng(sweeps)
    x, y, th = poses_around(rng, 3200, (0, 0, 0))
    out = check(eng, orc, w, bx, by, x, y, th, steps, sweeps)
    if steps == (0.0, 0.0):
        s0, c0 = orc.score_poses_det(w.meta, w.edt, bx, by, x, y, th)
        assert np.array_equal(bits(out[3]), bits(s0)) and np.array_equal(out[4], c0)


@pytest.mark.parametrize("n", [500, 3500])
def test_candidates_leaving_the_grid_on_every_side_and_poses_outside(eng, orc, room, n):
    """Poses along the four borders (their beams and some of their 27 candidates cross it), and poses far outside the grid,
    where every candidate scores 0 on 0 beams and nothing moves."""
    w, bx, by = room
    m = w.meta
    rng = np.random.default_rng(n)
    x0, x1 = m.min_x, m.min_x + m.pixel * (m.cols - 1)
    y0, y1 = m.min_y, m.min_y + m.pixel * (m.rows - 1)
    x, y, th = poses_around(rng, n, (0, 0, 0), (3.0, 3.0, 1.0))
    q = n // 5
    x[0:q] = x0 + rng.uniform(-0.2, 0.2, q)
    x[q:2 * q] = x1 + rng.uniform(-0.2, 0.2, q)
    y[2 * q:3 * q] = y0 + rng.uniform(-0.2, 0.2, q)
    y[3 * q:4 * q] = y1 + rng.uniform(-0.2, 0.2, q)
    far = slice(4 * q, 4 * q + q // 2)
    x[far] = rng.choice([-500.0, 500.0], q // 2)
    # short beams (a scan of nearby returns), so that the border poses keep some beams inside
    out = check(eng, orc, w, (bx * 0.02).astype(np.float32), (by * 0.02).astype(np.float32), x, y, th, COARSE, 2)
    assert np.array_equal(bits(out[0][far]), bits(x[far])) and not out[4][far].any() and not out[3][far].any()
    assert out[4][:4 * q].min() < out[4][:4 * q].max()   # in-bounds counts do vary along the borders


def test_float_path_on_a_grid_that_does_not_pack(eng, orc, room):
    """Values outside the packed code set (not sqrt of an integer): the engine keeps the float grid at every pose count."""
    w0, bx, by = room
    rng = np.random.default_rng(9)
    edt = (w0.edt * rng.uniform(0.9, 1.1, w0.edt.shape)).astype(np.float32)
    w = World(eng, w0.meta, edt)
    x, y, th = poses_around(rng, 3300, (0, 0, 0))
    check(eng, orc, w, bx, by, x, y, th, COARSE, 2)


@pytest.mark.parametrize("n", [200, 3200])
def test_no_pose_moves_on_an_all_free_grid(eng, orc, n):
    """Every cell at the cap, every beam of every candidate inside: 27 equal scores.  The incumbent keeps the centre; a
    kernel with FastMatch's first-candidate rule moves every pose to candidate 0."""
    import oracle
    rows = cols = 64
    w = World(eng, oracle.meta(rows, cols, cols, 0.1, -3.2, -3.2), np.full((rows, cols), 10.0, np.float32))
    rng = np.random.default_rng(3)
    bx, by = (rng.uniform(-1.2, 1.2, 40).astype(np.float32) for _ in range(2))
    x, y, th = (rng.uniform(-0.5, 0.5, n).astype(np.float32) for _ in range(3))
    for sweeps in (1, 5):
        out = check(eng, orc, w, bx, by, x, y, th, COARSE, sweeps)
        assert np.array_equal(bits(out[0]), bits(x)) and np.array_equal(bits(out[1]), bits(y)) and np.array_equal(bits(out[2]), bits(th))
        assert np.all(out[4] == 40)


@pytest.mark.parametrize("n,first_id,gather", [(300, 0, None), (3300, 1 << 33, None), (3300, 77, "shuffled"), (85, 5, "shuffled")])
def test_motion_refine_equals_motion_sample_then_refine(eng, orc, room, n, first_id, gather):
    """... with d_anc NULL and as a shuffled gather, first_id != 0; and the property that refinement never ends above the
    score slam_motion_score_dev gives the same sample (the centre is the incumbent)."""
    w, bx, by = room
    w.bind(eng)
    eng.scan_upload(bx, by)
    rng = np.random.default_rng(n)
    m = n + 11 if gather else n
    src = tuple(dev(a) for a in poses_around(rng, m, (0, 0, 0)))
    anc = dev(rng.integers(0, m, n).astype(np.int32)) if gather else None
    dp, sig, seed, frame = [0.01, -0.005, 0.002], [0.02, 0.02, 0.004], 4242, 3

    def buffers():
        return (tuple(torch.empty(n, device=DEV) for _ in range(3)), torch.empty(n, device=DEV),
                torch.empty(n, device=DEV, dtype=torch.int32))

    one, s1, c1 = buffers()
    eng.motion_refine_dev(1, src, anc, one, n, first_id, dp, sig, seed, frame, COARSE[0], COARSE[1], 2, s1, c1)
    two, s2, c2 = buffers()
    eng.motion_sample_dev(src, anc, two, n, first_id, dp, sig, seed, frame)
    eng.refine_poses_dev(1, two[0], two[1], two[2], n, COARSE[0], COARSE[1], 2, s2, c2)
    for a, b in zip(one + (s1,), two + (s2,)):
        assert np.array_equal(bits(host(a)), bits(host(b)))
    assert np.array_equal(host(c1), host(c2))
    plain, s0, c0 = buffers()
    eng.motion_score_dev(1, src, anc, plain, n, first_id, dp, sig, seed, frame, s0, c0)
    assert np.all(host(s1) <= host(s0))
    assert np.any(host(s1) < host(s0))


def test_error_codes(eng, room):
    pkg = load_package()
    w, bx, by = room
    w.bind(eng)
    eng.scan_upload(bx, by)
    n = 8
    x, y, th, sc = (torch.zeros(n, device=DEV) for _ in range(4))
    cn = torch.zeros(n, device=DEV, dtype=torch.int32)
    dst = tuple(torch.zeros(n, device=DEV) for _ in range(3))
    dp, sig = [0, 0, 0], [0.01, 0.01, 0.01]

    def status(fn):
        with pytest.raises(pkg.SlamError) as ei:
            fn()
        return ei.value.status

    INVALID, NOT_READY = -2, -4
    for sweeps in (0, 17, -1):
        assert status(lambda: eng.refine_poses_dev(1, x, y, th, n, 0.05, 0.01, sweeps, sc, cn)) == INVALID
        assert status(lambda: eng.motion_refine_dev(1, (x, y, th), None, dst, n, 0, dp, sig, 1, 0, 0.05, 0.01, sweeps, sc, cn)) == INVALID
    for t, r in ((-0.05, 0.01), (0.05, -0.01), (float("nan"), 0.01), (0.05, float("inf"))):
        assert status(lambda: eng.refine_poses_dev(1, x, y, th, n, t, r, 1, sc, cn)) == INVALID
        assert status(lambda: eng.motion_refine_dev(1, (x, y, th), None, dst, n, 0, dp, sig, 1, 0, t, r, 1, sc, cn)) == INVALID
    assert status(lambda: eng.refine_poses_dev(1, x, y, th, -1, 0.05, 0.01, 1, sc, cn)) == INVALID
    assert status(lambda: eng.refine_poses_dev(1, None, y, th, n, 0.05, 0.01, 1, sc, cn)) == INVALID
    assert status(lambda: eng.refine_poses_dev(1, x, y, th, n, 0.05, 0.01, 1, sc, None)) == INVALID
    assert status(lambda: eng.motion_refine_dev(1, (x, y, th), None, (x, y, th), n, 0, dp, sig, 1, 0, 0.05, 0.01, 1, sc, cn)) == INVALID
    assert status(lambda: eng.motion_refine_dev(1, (None, y, th), None, dst, n, 0, dp, sig, 1, 0, 0.05, 0.01, 1, sc, cn)) == INVALID
    assert status(lambda: eng.refine_poses_dev(3, x, y, th, n, 0.05, 0.01, 1, sc, cn)) == NOT_READY   # a slot nobody filled
    # n == 0 is fine and launches nothing
    eng.refine_poses_dev(1, None, None, None, 0, 0.05, 0.01, 1, None, None)
    eng.motion_refine_dev(1, (None, None, None), None, (None, None, None), 0, 0, dp, sig, 1, 0, 0.05, 0.01, 1, None, None)
    fresh = pkg.Engine(0)   # a grid but no scan yet / no grid
    try:
        assert status(lambda: fresh.refine_poses_dev(1, x, y, th, n, 0.05, 0.01, 1, sc, cn)) == NOT_READY
    finally:
        fresh.close()
