"""slam_localise_miss_dev / slam_localise_detcov_miss_dev (the misses of localisation in a known map, csrc/localise_kernels.hip)
against the specification tests/_localise_miss_spec.py: log-likelihood, stats, table and the three counts are equal exactly, in
both noise forms — on both sides of the staging seam, with the largest sight table beside the largest staged map and its table
row (the LDS budget's worst case), with and without a table pointer, with a persistent wavefront that takes two particles, under
every switch, on the edges the CPU test of the specification proves, and twice on the same buffers.  The entry points without
misses do not move the new counter."""
import numpy as np
import pytest
import torch

import _fov_spec as V
import _localise_miss_spec as MS
import _sight_spec as SS
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_localise import DEV, GATE, Q, dev, host, make_detections, make_map, make_poses, prepare
from test_gpu_localise_detcov import covariances, raw_map

pytestmark = pytest.mark.gpu
F = np.float32
PLAIN = (V.bound(-0.6), V.bound(1.9))      # lo <= hi
WRAP = (V.bound(-2.35), V.bound(2.35))     # lo > hi: the reference lidar's 269.5 degrees, blind behind


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for torch's fills and copies and the engine's launches
    yield e
    torch.cuda.synchronize()
    e.close()


def make_scan(seed, beams=360):
    """A ring of returns 2 to 14 m away: some landmarks lie in front of it, some behind."""
    rng = np.random.default_rng(seed)
    ang = np.linspace(-np.pi, np.pi, beams, endpoint=False)
    rad = rng.uniform(2.0, 14.0, beams)
    return (rad * np.cos(ang)).astype(F), (rad * np.sin(ang)).astype(F)


def run(eng, form, M, x, y, th, zx, zy, covs, view_range, arc, sight, scan, table, stride=None, counts=3):
    """One launch -> (assoc or None, stats, ll, missed, spared or None, outside or None)."""
    pkg = load_package()
    n, L = len(x), M.shape[1]
    Lp = (L + 31) // 32 * 32
    stride = L if stride is None else stride
    d_assoc = torch.full((n, stride), 7, dtype=torch.uint8, device=DEV) if table else None
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    d_ll = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
    d_cnt = [torch.full((n,), -7, dtype=torch.int32, device=DEV) if j < counts else None for j in range(3)]
    eng.detections_upload(zx, zy)
    if sight:
        eng.scan_upload(*scan)
        eng.sight_table_dev(sight[0])
    lo, hi = MS.ALL if arc is None else arc
    view = pkg.LocaliseView(view_range, float(lo), float(hi), 1 if sight else 0, sight[1] if sight else 0.0)
    if form == "detcov":
        eng.detections_cov_upload(*covs)
        eng.localise_detcov_miss_dev(raw_map(M, Lp), Lp, L, dev(x), dev(y), dev(th), n, GATE, d_assoc, stride, d_st, d_ll, view, *d_cnt)
    else:
        eng.localise_miss_dev(prepare(eng, M, Lp), Lp, L, dev(x), dev(y), dev(th), n, GATE, d_assoc, stride, d_st, d_ll, view, *d_cnt)
    return (host(d_assoc) if table else None, host(d_st), host(d_ll)) + tuple(host(c) if c is not None else None for c in d_cnt)


def check(eng, form, M, x, y, th, zx, zy, covs, view_range, arc, sight, scan, table=True, stride=None, label=""):
    L = M.shape[1]
    stride = L if stride is None else stride
    T = SS.table(scan[0], scan[1], sight[0]) if sight else None
    want = MS.localise(M, x, y, th, zx, zy, covs if form == "detcov" else Q, GATE, 0.0, 0.0, (view_range, arc, sight[1] if sight else None), T)
    got = run(eng, form, M, x, y, th, zx, zy, covs, view_range, arc, sight, scan, table, stride)
    if table:
        wt = np.concatenate([want[0], np.full((len(x), stride - L), 255, np.uint8)], axis=1)
        assert np.array_equal(got[0], wt), f"{label}: table differs at {np.argwhere(got[0] != wt)[:5].tolist()}"
    assert np.array_equal(got[1], want[1]), f"{label}: stats"
    assert np.array_equal(bits(got[2]), bits(want[2])), f"{label}: ll differs at {np.flatnonzero(bits(got[2]) != bits(want[2]))[:5].tolist()}"
    for j, name in ((3, "missed"), (4, "spared"), (5, "outside")):
        assert np.array_equal(got[j], want[j]), f"{label}: {name} differs at {np.flatnonzero(got[j] != want[j])[:5].tolist()}"
    return want


def big_n():
    """More particles than wavefronts can be resident at once (at most 8 workgroups of 4 a CU): some wavefront takes two."""
    return torch.cuda.get_device_properties(0).multi_processor_count * 32 + 65


# L, n, K, arc, sight (bins, margin), table, view_range.  2048 | 2049: the staging seam (the miss form keeps the stage's own; with
# 1024 bins and a table row L = 2048 is the 64 KB worst case); 8192: the largest map; n = None: big_n()
CASES = (
    (1, 1, 1, None, None, True, 30.0),
    (64, 65, 16, PLAIN, (32, 0.5), False, 12.0),
    (127, 65, 64, WRAP, (1024, 0.5), True, 12.0),
    (128, 65, 0, PLAIN, None, True, 12.0),
    (129, 130, 16, WRAP, (32, 0.5), True, 12.0),
    (129, 65, 1, None, (1024, 0.5), False, 12.0),
    (500, 65, 16, WRAP, (1024, 0.5), False, 9.0),
    (2048, 65, 16, WRAP, (1024, 0.5), True, 9.0),
    (2048, 65, 64, None, None, False, 9.0),
    (2049, 65, 16, PLAIN, (1024, 0.5), True, 9.0),
    (8192, 8, 64, WRAP, (1024, 0.5), True, 6.0),
    (129, None, 4, WRAP, (32, 0.5), False, 12.0),
)


@pytest.mark.parametrize("form", ("iso", "detcov"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"L{c[0]}-n{c[1]}-K{c[2]}")
def test_equals_the_spec(eng, case, form):
    L, n, K, arc, sight, table, view_range = case
    n = big_n() if n is None else n
    M = make_map(L, 300 + L)
    true, x, y, th = make_poses(n, L + K)
    th = (th + np.linspace(0.0, 6.0, n)).astype(F)   # headings all round: every landmark is ahead of some, behind others
    zx, zy = make_detections(M, true, K, 7 * L + K)
    want = check(eng, form, M, x, y, th, zx, zy, covariances(K, 11 * L + K), view_range, arc, sight, make_scan(L + n), table,
                 stride=(L + 35) // 32 * 32 if K % 2 == 0 else L + 3, label=f"{form} L={L} n={n} K={K}")
    _, stats, _, missed, spared, outside = want
    if L >= 64:   # (the case exercises what it is there for)
        assert missed.sum() > 0
        assert (outside.sum() > 0) == (arc is not None) and (spared.sum() > 0) == (sight is not None)
    if K >= 16 and n >= 65:
        assert stats[:, 0].sum() > 0


def edge_case():
    """The edges of test_localise_miss_spec_cpu.py in one map, seen from the origin with heading 0 (particle 0), from a pose that
    sits ON landmark 2 (1), from NaN poses (2: x, 3: theta) and from a pose that matches landmark 0 (4)."""
    r = F(5.0)
    pts = [(5.0, 0.0), (float(np.nextafter(r, F(np.inf))), 0.0), (1.25, 3.5), (1.0, 1.0), (2.0, 0.0), (2.0, 0.3), (-2.0, 0.0), (0.0, -2.0),
           (3.0, 3.0)]
    M = np.zeros((5, len(pts)), np.float32)
    M[0], M[1] = np.array(pts, np.float32).T
    M[2], M[4] = 0.05, 0.05
    M[2, 8] = -1.0   # an unseen slot
    x = np.array([0.0, 1.25, np.nan, 0.0, 0.0], F)
    y = np.array([0.0, 3.5, 0.0, 0.0, 0.0], F)
    th = np.array([0.0, 0.7, 0.0, np.nan, 0.0], F)
    return M, x, y, th


@pytest.mark.parametrize("form", ("iso", "detcov"))
def test_the_edges_of_the_predicate(eng, form):
    M, x, y, th = edge_case()
    zx, zy = np.array([5.0], F), np.array([0.0], F)   # landmark 0 as the origin sees it
    covs = covariances(1, 3)
    p = F(0.5)                                        # the diamond angle of (1, 1)
    j = int(SS.bin_of(np.array([2.0], F), np.array([0.3], F), 32)[0][0])
    views = [(5.0, None, None, None), (5.0, (p, F(1.0)), None, None), (5.0, (F(0.0), p), None, None),
             (5.0, (np.nextafter(p, F(4)), F(1.0)), None, None), (5.0, (F(3.0), F(1.0)), None, None)]
    # a scan that hit 0.5 m ahead: (2, 0) against margins 2 (g == 0: not hidden) and 1 (hidden); (2, 0.3) hidden through a neighbour bin only
    ahead = (np.array([0.5], F), np.array([0.0], F))
    views += [(5.0, None, (32, 2.0), ahead), (5.0, None, (32, 1.0), ahead), (5.0, (F(3.0), F(1.0)), (32, 1.0), ahead)]
    for d in (-1, 1):
        a = ((j + d) % 32 + 0.5) / 8.0               # a diamond angle in the middle of the neighbour bin, first quadrant
        views.append((5.0, None, (32, 0.5), (np.array([0.5 * (1 - a)], F), np.array([0.5 * a], F))))
    seen_any = np.zeros(3, np.int64)
    for view_range, arc, sight, scan in views:
        want = check(eng, form, M, x, y, th, zx, zy, covs, view_range, arc, sight, scan, label=f"{form} {arc} {sight}")
        assert want[3][2] == 0 and want[4][2] == 0 and want[5][2] == 0   # the NaN pose counts nothing
        assert want[1][0, 0] == 1 and want[1][4, 0] == 1                # the origin matches landmark 0: it is no miss
        seen_any += [want[3].sum(), want[4].sum(), want[5].sum()]
    assert np.all(seen_any > 0)


def test_nothing_detected_and_everything_matched(eng):
    L = 40
    M = make_map(L, 77, unseen=0.3)
    seen = ~(M[2] < 0)
    x, y, th = np.array([1.5], F), np.array([-2.0], F), np.array([0.7], F)
    none = np.zeros(0, F)
    want = check(eng, "iso", M, x, y, th, none, none, None, 100.0, None, None, None, label="K = 0")
    assert want[3][0] == seen.sum()
    c, s = np.cos(0.7), np.sin(0.7)
    dx, dy = M[0, seen].astype(np.float64) - 1.5, M[1, seen].astype(np.float64) + 2.0
    zx, zy = (c * dx - s * dy).astype(F), (s * dx + c * dy).astype(F)
    want = check(eng, "iso", M, x, y, th, zx, zy, None, 100.0, None, None, None, label="all matched")
    assert want[1][0, 0] == seen.sum() and want[3][0] == 0


def test_a_second_call_and_optional_counts(eng):
    L, n, K = 129, 65, 16
    M = make_map(L, 81)
    true, x, y, th = make_poses(n, 82)
    zx, zy = make_detections(M, true, K, 83)
    covs, scan = covariances(K, 84), make_scan(85)
    for form in ("iso", "detcov"):
        a = run(eng, form, M, x, y, th, zx, zy, covs, 12.0, WRAP, (64, 0.5), scan, True)
        b = run(eng, form, M, x, y, th, zx, zy, covs, 12.0, WRAP, (64, 0.5), scan, True)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8))
        c = run(eng, form, M, x, y, th, zx, zy, covs, 12.0, WRAP, (64, 0.5), scan, False, counts=1)   # spared, outside: NULL
        assert c[4] is None and c[5] is None and np.array_equal(c[3], a[3]) and np.array_equal(bits(c[2]), bits(a[2]))


def test_argument_checks_and_counters(eng):
    pkg = load_package()
    L, Lp, n = 64, 64, 8
    M = make_map(L, 51)
    true, x, y, th = make_poses(n, 52)
    zx, zy = make_detections(M, true, 4, 53)
    covs = covariances(4, 54)
    d_prep, d_raw = prepare(eng, M, Lp), raw_map(M, Lp)
    d_st = torch.zeros((n, 3), dtype=torch.int32, device=DEV)
    d_ms = torch.zeros((n,), dtype=torch.int32, device=DEV)
    eng.detections_upload(zx, zy)
    eng.detections_cov_upload(*covs)
    before = (eng.localise_counts(), eng.localise_detcov_count(), eng.localise_miss_count())
    # the entry points without misses move their own counters only
    eng.localise_dev(d_prep, Lp, L, dev(x), dev(y), dev(th), n, GATE, None, L, d_st, None)
    eng.localise_detcov_dev(d_raw, Lp, L, dev(x), dev(y), dev(th), n, GATE, None, L, d_st, None)
    assert eng.localise_miss_count() == before[2]
    ok = pkg.LocaliseView(5.0, 0.0, 4.0, 0, 0.0)
    for fn, d_map in ((eng.localise_miss_dev, d_prep), (eng.localise_detcov_miss_dev, d_raw)):
        call = lambda view, missed=d_ms: fn(d_map, Lp, L, dev(x), dev(y), dev(th), n, GATE, None, L, d_st, None, view, missed)
        for bad in (dict(view_range=0.0), dict(view_range=-1.0), dict(view_range=float("inf")), dict(view_range=float("nan")),
                    dict(lo=-0.5), dict(hi=4.5), dict(lo=float("nan")), dict(sight=1, margin=0.0), dict(sight=1, margin=float("nan")),
                    dict(sight=1, margin=float("inf"))):
            kw = dict(view_range=5.0, lo=0.0, hi=4.0, sight=0, margin=0.0)
            kw.update(bad)
            with pytest.raises(pkg.SlamError):
                call(pkg.LocaliseView(kw["view_range"], kw["lo"], kw["hi"], kw["sight"], kw["margin"]))
        with pytest.raises(pkg.SlamError):
            call(None)
        with pytest.raises(pkg.SlamError):
            call(ok, None)
        eng.scan_upload(*make_scan(1))   # a new scan drops the sight table: sight on is not ready
        with pytest.raises(pkg.SlamError) as err:
            call(pkg.LocaliseView(5.0, 0.0, 4.0, 1, 0.5))
        assert err.value.status == -4   # SLAM_ERR_NOT_READY
    assert (eng.localise_counts(), eng.localise_detcov_count()) == ((before[0][0], before[0][1] + 1), before[1] + 1)
    assert eng.localise_miss_count() == before[2]
    call(ok)
    assert eng.localise_miss_count() == before[2] + 1
    assert (eng.localise_counts(), eng.localise_detcov_count()) == ((before[0][0], before[0][1] + 1), before[1] + 1)
