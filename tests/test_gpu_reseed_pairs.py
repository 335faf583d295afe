"""slam_pose_reseed_pairs_dev (reseeding from detection pairs, csrc/reseed_pair_kernels.hip) against the specification
tests/_reseed_pair_spec.py: poses bit for bit, flags and the four counts exactly — at the smallest shapes at which the kernel can go
wrong: one slot, a wavefront less one, exactly one, one more, more than a workgroup, several with a ragged tail; maps of 2, 63, 64,
65 and 130 landmarks, so the 64-lane scan meets a ragged chunk alone, a full one, a full and a ragged one, and a third; maps built
so that a slot has no partner, exactly one, 64 in one chunk, partners in the last ragged chunk only, or every landmark but its own;
empty slots; the inclusive bounds on integers; two detections and sixty-four; every fraction; a particle id past 2^32; in place
without a gather and out of place through one; both plane strides; coordinates out to 10^3 — and its refusals."""
import itertools

import numpy as np
import pytest
import torch

import _reseed_pair_spec as RP
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_reseed import make_anc, make_poses

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SEED = 0x0FED_CBA9_8765_4321
INVALID_ARG, NOT_READY = -2, -4
CENTRE = np.array([900.0, -950.0])
RADIUS = 7.0
LS = (2, 63, 64, 65, 130)
COMBOS = list(itertools.product((2, 64), (1.0 / 16, 0.5, 1.0), (0, 2**32 + 7), (False, True), (False, True)))


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for torch's fills and copies and the engine's launches
    yield e
    torch.cuda.synchronize()
    e.close()


def blank(L):
    M = np.zeros((5, L), F)
    M[2], M[3], M[4] = 0.05, 0.01, 0.08
    return M


def two_points(K, r):
    """K detections on two spots r apart (even k on one, odd k on the other): a pair is r apart or on one spot (too close)."""
    odd = (np.arange(K) % 2).astype(np.float64)
    return (1.0 + 0.6 * r * odd).astype(F), (2.0 + 0.8 * r * odd).astype(F)


def lattice(L, K, empty):
    """L landmarks on a shuffled unit lattice near CENTRE, seen from a pose with 2 cm of noise: K of them, with repeats (pairs on
    one landmark are too close).  Distances such as 5 and sqrt 5 have many partners, others none.  tol 0.3, min_sep 0.8."""
    rng = np.random.default_rng(31 + L)
    side = int(np.ceil(np.sqrt(L))) + 2
    cells = rng.permutation(side * side)[:L]
    M = blank(L)
    M[0], M[1] = CENTRE[0] + cells % side, CENTRE[1] + cells // side
    if empty:
        M[2, ::3] = -1.0
    seen = rng.integers(0, L, K)
    t = 0.9
    dx, dy = M[0][seen].astype(np.float64) - (CENTRE[0] + 1.3), M[1][seen].astype(np.float64) - (CENTRE[1] - 0.6)
    zx = np.cos(t) * dx - np.sin(t) * dy + 0.02 * rng.standard_normal(K)
    zy = np.sin(t) * dx + np.cos(t) * dy + 0.02 * rng.standard_normal(K)
    return M, zx.astype(F), zy.astype(F), 0.3, 0.8


def line(L, K):
    """Landmarks 0 .. L-2 on a line 100 m apart, the last one RADIUS from landmark 0: with detections RADIUS apart landmark 0 has
    exactly one partner, in the last (ragged) chunk, the last landmark has landmark 0, and every other landmark has none."""
    M = blank(L)
    M[0, :L - 1], M[1, :L - 1] = CENTRE[0] - 100.0 * np.arange(L - 1), CENTRE[1]
    M[0, L - 1], M[1, L - 1] = CENTRE[0], CENTRE[1] + RADIUS
    return (M,) + two_points(K, RADIUS) + (0.01, 1.0)


def polygon(L, K):
    """Landmark 0 in the middle of a regular (L-1)-gon of radius RADIUS: every landmark but itself is its partner."""
    M = blank(L)
    ang = 2 * np.pi * np.arange(L - 1) / (L - 1) + 0.1
    M[0, 0], M[1, 0] = CENTRE
    M[0, 1:], M[1, 1:] = CENTRE[0] + RADIUS * np.cos(ang), CENTRE[1] + RADIUS * np.sin(ang)
    return (M,) + two_points(K, RADIUS) + (0.01, 1.0)


def ring64(K):
    """130 landmarks: landmark 129 in the middle of a ring of the 64 landmarks 64 .. 127 — its 64 partners fill the second chunk, all
    64 lanes of one ballot; the first chunk and landmark 128 lie far away (on the line of `line`)."""
    M = line(130, K)[0]
    ang = 2 * np.pi * np.arange(64) / 64 + 0.05
    mid = CENTRE + (300.0, 400.0)
    M[0, 129], M[1, 129] = mid
    M[0, 64:128], M[1, 64:128] = mid[0] + RADIUS * np.cos(ang), mid[1] + RADIUS * np.sin(ang)
    M[0, 128], M[1, 128] = CENTRE[0] + 50.0, CENTRE[1] - 777.0
    return (M,) + two_points(K, RADIUS) + (0.01, 1.0)


def integers(K):
    """tol = 0 on integer coordinates (test_reseed_pair_spec_cpu.py): detections 5 apart (3-4-5); from landmarks 0 and 5, on one
    spot, (3, 4), (5, 0) and (4, 3) are partners with dm2 on both inclusive bounds, (6, 0) and the twin are not."""
    off = np.array([(0, 0), (3, 4), (5, 0), (4, 3), (6, 0), (0, 0)], np.float64)
    M = blank(6)
    M[0], M[1] = 10.0 + off[:, 0], 20.0 + off[:, 1]
    odd = (np.arange(K) % 2).astype(F)
    return M, (1.0 + 3.0 * odd).astype(F), (2.0 + 4.0 * odd).astype(F), 0.0, 1.0


def cases():
    """(label, wanted partner counts, builder(K)) — wanted: partner counts some searching slot of the case must have (checked on the
    specification wherever enough slots are chosen to expect them)."""
    out = []
    for L in LS:
        out.append((f"lattice L {L}", (), lambda K, L=L: lattice(L, K, False)))
        out.append((f"lattice with empty slots L {L}", (), lambda K, L=L: lattice(L, K, True)))
        out.append((f"line L {L}", (1,) if L == 2 else (0, 1), lambda K, L=L: line(L, K)))
        out.append((f"polygon L {L}", (L - 1,), lambda K, L=L: polygon(L, K)))
    out.append(("ring of 64 in the second chunk", (64, 0), ring64))
    out.append(("integers, tol 0", (3, 1), integers))
    return out


def partner_counts(M, zx, zy, n, first_id, frame, tol, min_sep, flag):
    """the specification's cnt of every slot that searched (flag 1 or 4)"""
    r0, j1, k1, k2, rb0 = RP.draws(n, first_id, SEED, frame, M.shape[1], len(zx))
    out = []
    for i in np.flatnonzero((flag == 1) | (flag == 4)):
        ax, ay = zx[k2[i]] - zx[k1[i]], zy[k2[i]] - zy[k1[i]]
        dz = np.sqrt(ax * ax + ay * ay)
        lo, hi = dz - F(tol), dz + F(tol)
        out.append(int(RP.partners(M, j1[i], lo * lo, hi * hi).sum()))
    return out


def padded(M, Lp):
    raw = np.full((5, Lp), np.nan, F)   # the padding behind nlandmarks is never read: NaN would show
    raw[:, :M.shape[1]] = M
    return raw


def run(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction, tol, min_sep, wide=False, flag=True):
    """-> (x', y', th', flag, counts): in place when anc is None, else into buffers of their own.  wide: a plane stride well beyond
    the landmarks (else the landmarks exactly: no padding at all)."""
    n, L = len(x), M.shape[1]
    Lp = (L + 31) // 32 * 32 + 32 if wide else L
    d_in = [dev(a) for a in (x, y, th)]
    d_out = d_in if anc is None else [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_flag = torch.full((n,), 9, dtype=torch.uint8, device=DEV) if flag else None
    eng.detections_upload(zx, zy)
    counts = eng.pose_reseed_pairs_dev(dev(padded(M, Lp)), Lp, L, *d_in, None if anc is None else dev(anc), *d_out, n, first_id, SEED,
                                       frame, fraction, tol, min_sep, d_flag)
    if anc is not None:   # the inputs are read only
        assert all(np.array_equal(bits(host(d)), bits(a)) for d, a in zip(d_in, (x, y, th)))
    return [host(d) for d in d_out] + [host(d_flag) if flag else None, counts]


def check(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction, tol, min_sep, wide, label):
    want = RP.reseed_pairs(M, x, y, th, anc, zx, zy, first_id, SEED, frame, fraction, tol, min_sep)
    got = run(eng, M, x, y, th, anc, zx, zy, first_id, frame, fraction, tol, min_sep, wide)
    assert np.array_equal(got[3], want[3]), f"{label}: flags differ at {np.flatnonzero(got[3] != want[3])[:5].tolist()}"
    for k, name in enumerate(("x", "y", "theta")):
        assert np.array_equal(bits(got[k]), bits(want[k])), f"{label}: {name} differs at {np.flatnonzero(bits(got[k]) != bits(want[k]))[:5].tolist()}"
    assert got[4] == tuple(want[4]), f"{label}: counts {got[4]} != {tuple(want[4])}"
    return want


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1000])
def test_stage_equals_the_spec(eng, n):
    x, y, th = make_poses(n)
    anc = make_anc(n)
    totals = np.zeros(4, np.int64)
    kept = 0
    for c, (label, wanted, build) in enumerate(cases()):
        K, fraction, first_id, gather, wide = COMBOS[(7 * c + 5 * n) % len(COMBOS)]
        M, zx, zy, tol, min_sep = build(K)
        want = check(eng, M, x, y, th, anc if gather else None, zx, zy, first_id, c, fraction, tol, min_sep, wide,
                     f"n {n} {label} K {K} fraction {fraction} first_id {first_id} gather {gather} wide {wide}")
        totals += want[4]
        kept += n - int(want[4].sum())
    if n >= 63:
        assert np.all(totals > 0) and kept > 0, totals   # every branch of a slot was taken


@pytest.mark.parametrize("label, wanted, build", cases(), ids=[c[0] for c in cases()])
def test_every_lane_of_a_wavefront_is_served(eng, label, wanted, build):
    """Fraction 1: all 64 lanes of every wavefront are chosen, and served one after another, with 2 detections and with 64, through
    the gather; and among that many slots the partner counts the case was built for do turn up (counted on the specification)."""
    n = 1000
    x, y, th = make_poses(n)
    cnt = set()
    for frame, K in enumerate((2, 64)):
        M, zx, zy, tol, min_sep = build(K)
        want = check(eng, M, x, y, th, make_anc(n), zx, zy, 2**32 + 7, frame, 1.0, tol, min_sep, True, f"{label} K {K}")
        assert np.all(want[3] != 0)
        cnt |= set(partner_counts(M, zx, zy, n, 2**32 + 7, frame, tol, min_sep, want[3]))
    assert set(wanted) <= cnt, f"{label}: partner counts {sorted(cnt)} lack {wanted}"


def test_counts_are_left_clean_and_launches_counted(eng):
    """The same launch again gives the same counts (the accumulators and the ticket were cleared); no flag pointer; the launches
    go into slam_pose_reseed_pairs_count and not into slam_pose_reseed_count."""
    n = 1000
    x, y, th = make_poses(n)
    M, zx, zy, tol, min_sep = lattice(65, 64, True)
    c0, s0 = eng.pose_reseed_pairs_count(), eng.pose_reseed_count()
    for frame in (3, 3, 4):
        want = check(eng, M, x, y, th, make_anc(n), zx, zy, 2**32 + 7, frame, 0.5, tol, min_sep, False, f"frame {frame}")
        assert np.all(want[4] > 0)
    got = run(eng, M, x, y, th, None, zx, zy, 0, 5, 0.5, tol, min_sep, flag=False)
    want = RP.reseed_pairs(M, x, y, th, None, zx, zy, 0, SEED, 5, 0.5, tol, min_sep)
    assert all(np.array_equal(bits(got[k]), bits(want[k])) for k in range(3)) and got[4] == tuple(want[4])
    assert eng.pose_reseed_pairs_count() - c0 == 4 and eng.pose_reseed_count() == s0


def test_refusals(eng):
    pkg = load_package()
    n, L, Lp = 64, 5, 32
    x, y, th = make_poses(n)
    M, zx, zy, tol, min_sep = polygon(L, 4)
    d_map = dev(padded(M, Lp))
    d_in = [dev(a) for a in (x, y, th)]
    d_out = [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_anc = dev(make_anc(n))
    d_big = torch.zeros(4 * n, dtype=torch.float32, device=DEV)
    eng.detections_upload(zx, zy)
    c0 = eng.pose_reseed_pairs_count()

    def call(map_=d_map, ps=Lp, nl=L, ins=d_in, anc=None, outs=d_out, n_=n, fraction=0.5, tol_=tol, sep=min_sep):
        return eng.pose_reseed_pairs_dev(map_, ps, nl, *ins, anc, *outs, n_, 0, SEED, 0, fraction, tol_, sep)

    nan, inf = float("nan"), float("inf")
    bad = [dict(n_=0), dict(n_=-3), dict(nl=0), dict(nl=-1), dict(nl=1), dict(ps=L - 1), dict(fraction=0.0), dict(fraction=-0.25),
           dict(fraction=1.5), dict(fraction=nan), dict(fraction=inf), dict(map_=None), dict(ins=[None, d_in[1], d_in[2]]),
           dict(outs=[d_out[0], None, d_out[2]]),
           dict(tol_=-0.01), dict(tol_=nan), dict(tol_=inf), dict(tol_=inf, sep=inf), dict(tol_=1.0, sep=1.0), dict(tol_=1.0, sep=0.5),
           dict(sep=nan), dict(sep=inf), dict(sep=0.0, tol_=0.0),
           dict(anc=d_anc, outs=d_in),                                        # in place through a gather
           dict(outs=[d_in[1], d_out[1], d_out[2]]),                          # x_out is y_in
           dict(ins=[d_big[:n], d_big[n:2 * n], d_big[2 * n:3 * n]], outs=[d_big[1:n + 1], d_out[1], d_out[2]]),   # shifted by one float
           dict(anc=d_anc, ins=[d_big[:n], d_big[n:2 * n], d_big[2 * n:3 * n]], outs=[d_big[n - 1:2 * n - 1], d_out[1], d_out[2]])]
    for kw in bad:
        with pytest.raises(pkg.SlamError) as err:
            call(**kw)
        assert err.value.status == INVALID_ARG, kw
    assert eng.pose_reseed_pairs_count() == c0 and all(np.all(host(d) == 7.0) for d in d_out)
    assert sum(call()) > 0 and eng.pose_reseed_pairs_count() == c0 + 1            # the good call, out of place without a gather
    assert sum(call(anc=d_anc)) > 0 and sum(call(outs=d_in)) > 0                 # ... through one; in place without
    assert sum(call(tol_=0.0, sep=1e-30)) > 0                                    # the least the parameters may be

    fresh = pkg.Engine(0)   # no detections were ever handed over
    with pytest.raises(pkg.SlamError) as err:
        fresh.pose_reseed_pairs_dev(d_map, Lp, L, *d_in, None, *d_out, n, 0, SEED, 0, 0.5, tol, min_sep)
    assert err.value.status == NOT_READY
    with pytest.raises(pkg.SlamError) as err:   # ... and an invalid argument is still one
        fresh.pose_reseed_pairs_dev(d_map, Lp, L, *d_in, None, *d_out, 0, 0, SEED, 0, 0.5, tol, min_sep)
    assert err.value.status == INVALID_ARG
    torch.cuda.synchronize()
    fresh.close()


@pytest.mark.parametrize("K", [0, 1])
def test_fewer_than_two_detections_write_nothing(eng, K):
    n, L, Lp = 257, 5, 32
    x, y, th = make_poses(n)
    d_out = [torch.full((n,), 7.0, dtype=torch.float32, device=DEV) for _ in range(3)]
    d_flag = torch.full((n,), 9, dtype=torch.uint8, device=DEV)
    eng.detections_upload(np.ones(K, F), np.ones(K, F))
    c0 = eng.pose_reseed_pairs_count()
    counts = eng.pose_reseed_pairs_dev(dev(padded(polygon(L, 2)[0], Lp)), Lp, L, dev(x), dev(y), dev(th), None, *d_out, n, 0, SEED, 0, 1.0,
                                       0.01, 1.0, d_flag)
    assert counts == (0, 0, 0, 0) and eng.pose_reseed_pairs_count() == c0
    assert all(np.all(host(d) == 7.0) for d in d_out) and np.all(host(d_flag) == 9)
