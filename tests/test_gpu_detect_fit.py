"""slam_detect_scan_fit_dev (the fitted landmark detector, csrc/detect_kernels.hip) against its specification
tests/_detect_fit_spec.py: zx, zy, ndet and all four stats are equal bit for bit at the scan sizes around the kernel's lane,
wavefront and round boundaries, with and without wrap, on random pole fields, on the hand-made scans of the centroid detector
(tests/_detect_scenes.py) and of the fit's own edges (tests/_detect_fit_scenes.py), on arcs of 64 points across a mask word and
across the end of the scan; without a fit the new entry point is slam_detect_scan_dev; the counter, the pending count and the
argument checks."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
import _detect_fit_scenes as FS
import _detect_fit_spec as DF
import _detect_scenes as S
import _detect_spec as D
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_aniso import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PS = (0, 1, 2, 63, 64, 65, 256, 257, 360, 4096)
FITS = ((0.1, 0.0), (0.07, 0.05))
SCENES = S.scenarios()
FIT_SCENES = FS.scenarios()
GUARD = -77


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


def run(eng, bx, by, kw, fit, through_old=False):
    eng.scan_upload(bx, by)
    d = torch.full((12,), GUARD, dtype=torch.int32, device=DEV)   # guard words before and behind the four stats
    if through_old:
        eng.detect_scan_dev(d_stats=d[4:8], **kw)
    else:
        eng.detect_scan_fit_dev(fit, d_stats=d[4:8], **kw)
    zx, zy, ndet = eng.detections(full=True)
    return zx, zy, ndet, host(d)


def check(eng, bx, by, kw, fit, label):
    """One launch against the spec -> the spec's (zx, zy, ndet, stats)."""
    want = DF.detect_fit(bx, by, fit, **kw)
    zx, zy, ndet, st = run(eng, bx, by, kw, fit)
    print(f"{label}: P={len(bx)} fit={fit} stats={st[4:8].tolist()} want={want[3].tolist()}")
    assert ndet == want[2], f"{label}: ndet {ndet} != {want[2]}"
    assert np.array_equal(st[4:8], want[3]), f"{label}: stats {st[4:8].tolist()} != {want[3].tolist()}"
    assert np.all(st[:4] == GUARD) and np.all(st[8:] == GUARD), f"{label}: written beside the stats"
    assert np.array_equal(bits(zx), bits(want[0])) and np.array_equal(bits(zy), bits(want[1])), f"{label}: detections"
    assert not bits(zx[ndet:]).any() and not bits(zy[ndet:]).any(), f"{label}: entries behind ndet"
    return want


@pytest.mark.parametrize("P", PS)
def test_pole_fields(eng, P):
    """The fields' poles are runs of 1 .. 7 points about 0.04 .. 0.09 m apart: some rounder than a circle of 0.1 m allows, some not,
    one across the end of the scan (cut without wrap)."""
    accepted = shape = 0
    for wrap in (1, 0):
        for fit in FITS:
            bx, by, kw = S.pole_field(P, 100 + P)
            want = check(eng, bx, by, dict(kw, wrap=wrap), fit, f"P={P} wrap={wrap}")
            accepted += int(want[3][1])
            shape += int(want[3][3])
    if P >= 63:
        assert accepted > 0
    if P >= 256:
        assert shape > 0
    if P == 4096:                       # the cap: a radius that takes most poles, the first 64 by start index
        want = check(eng, bx, by, kw, (0.3, 0.0), f"P={P}, the cap")
        assert want[3][1] > 64 and want[2] == 64


def test_the_wrap_pole_is_fitted_through_the_end_of_the_scan(eng):
    bx, by, kw = S.pole_field(360, 460)
    with_wrap = check(eng, bx, by, kw, (0.2, 0.0), "wrap")
    without = check(eng, bx, by, dict(kw, wrap=0), (0.2, 0.0), "no wrap")
    assert with_wrap[3][1] + with_wrap[3][3] == without[3][1] + without[3][3] + 1


@pytest.mark.parametrize("name", sorted(SCENES))
def test_centroid_scenarios_under_a_fit(eng, name):
    bx, by, kw, _ = SCENES[name]
    for fit in ((0.1, 0.0), (0.25, 0.1)):
        check(eng, bx, by, kw, fit, name)


@pytest.mark.parametrize("name", sorted(FIT_SCENES))
def test_fit_scenarios(eng, name):
    bx, by, kw, fit, stats = FIT_SCENES[name]
    want = check(eng, bx, by, kw, fit, name)
    assert want[3].tolist() == stats


@pytest.mark.parametrize("lead, roll", [(3, 0), (30, 0), (62, 0), (3, -40), (130, -170)])
def test_an_arc_of_64_points(eng, lead, roll):
    """max_points = 64 and a segment of exactly 64 points: inside one mask word's reach, across a word seam, through P - 1 into 0."""
    bx, by, kw = FS.arc_scene(lead, roll=roll)
    for wrap in (1, 0):
        want = check(eng, bx, by, dict(kw, wrap=wrap), (0.1, 0.0), f"arc lead={lead} roll={roll} wrap={wrap}")
        assert want[2] == (1 if wrap or roll == 0 else 0)
    bx, by, kw = FS.arc_scene(lead, m=65, roll=roll)
    assert check(eng, bx, by, kw, (0.1, 0.0), "arc of 65")[2] == 0


@pytest.mark.parametrize("P", (256, 1088))
def test_segments_across_every_word_boundary(eng, P):
    """A pole of six points across every multiple of 64 and, cyclically, across the end of the scan."""
    R = 0.1 * P / (2 * np.pi)
    r = np.full(P, R)
    for c in range(0, P, 64):
        r[np.arange(c - 3, c + 3) % P] = 0.7 * R
    a = -np.pi + 2 * np.pi * np.arange(P) / P
    bx, by = (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)
    kw = dict(D.DEFAULTS, max_range=1000.0)
    want = check(eng, bx, by, kw, (0.15, 0.0), f"boundaries P={P}")
    assert want[3][1] == P // 64 and want[3][3] == 0
    want = check(eng, bx, by, dict(kw, wrap=0), (0.15, 0.0), f"boundaries P={P} wrap=0")
    assert want[3][1] == P // 64 - 1
    want = check(eng, bx, by, kw, (0.1, 0.0), f"boundaries P={P}, too wide for 0.1")
    assert want[3][1] == 0 and want[3][3] == P // 64


def test_without_a_fit_it_is_slam_detect_scan_dev(eng):
    for P in (65, 360, 4096):
        bx, by, kw = S.pole_field(P, 7 + P)
        c0, f0 = eng.detect_count(), eng.detect_fit_count()
        new = run(eng, bx, by, kw, None)
        old = run(eng, bx, by, kw, None, through_old=True)
        assert (eng.detect_count(), eng.detect_fit_count()) == (c0 + 2, f0)          # two launches, none of them a fit
        assert new[2] == old[2] > 0 and np.array_equal(new[3], old[3]) and new[3][7] == 0
        assert np.array_equal(bits(new[0]), bits(old[0])) and np.array_equal(bits(new[1]), bits(old[1]))
        run(eng, bx, by, kw, (0.1, 0.0))
        assert (eng.detect_count(), eng.detect_fit_count()) == (c0 + 3, f0 + 1)


def test_pending_count_reaches_the_association(eng):
    """slam_associate_dev right after slam_detect_scan_fit_dev = after slam_detections_upload_host of the spec's output."""
    n, L, Lp = 65, 100, 128
    poses, rows, _, _ = make_case(n, L, Lp, 21)
    bx, by, kw = S.pole_field(360, 9)
    fit = (0.2, 0.0)
    zx, zy, k, _ = DF.detect_fit(bx, by, fit, **kw)
    assert 3 < k < 64

    def associate():
        d_assoc = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
        d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
        eng.associate_dev(dev(rows), 5 * Lp, Lp, L, dev(poses[0]), dev(poses[1]), dev(poses[2]), None, n, 0.02, 9.21, 50.0, 1, d_assoc, Lp,
                          d_st)
        return host(d_assoc), host(d_st)

    eng.scan_upload(bx, by)
    eng.detect_scan_fit_dev(fit, **kw)
    got = associate()
    eng.detections_upload(zx[:k], zy[:k])
    want = associate()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    spec = A.associate(rows, *poses, None, zx[:k], zy[:k], 0.02, 9.21, 50.0, 1, L=L, assoc_stride=Lp)
    assert np.array_equal(got[0], spec[0]) and np.array_equal(got[1], spec[1])
    assert int(got[1][:, :2].sum()) > 0


def test_argument_checks_and_the_counters(eng):
    pkg = load_package()
    bx, by, kw = S.pole_field(64, 1)
    eng.scan_upload(bx, by)
    c0, f0, a0 = eng.detect_count(), eng.detect_fit_count(), eng.assoc_counts()
    for bad in ((0.0, 0.0), (-0.1, 0.0), (float("nan"), 0.0), (float("inf"), 0.0), (0.1, -1e-3), (0.1, float("nan")), (0.1, float("inf"))):
        assert not DF.fit_ok(bad)
        with pytest.raises(pkg.SlamError) as err:
            eng.detect_scan_fit_dev(bad)
        assert err.value.status == -2 and "radius" in str(err.value), bad
    with pytest.raises(pkg.SlamError) as err:                    # the parameters are checked as before
        eng.detect_scan_fit_dev((0.1, 0.0), min_points=0)
    assert err.value.status == -2 and "min_points" in str(err.value)
    assert eng.lib.slam_detect_scan_fit_dev(eng.h, None, None, None) == -2
    assert eng.lib.slam_detect_fit_count(eng.h, None) == -2
    assert (eng.detect_count(), eng.detect_fit_count()) == (c0, f0)
    f = pkg.DetectFit.default()
    assert (round(f.radius, 6), f.spread_tol) == (0.1, 0.0)
    eng.detect_scan_fit_dev(f)                                   # d_stats may be NULL
    eng.detect_scan_fit_dev(pkg.DetectFit.default(radius=0.3, spread_tol=0.1), **kw)
    assert (eng.detect_count(), eng.detect_fit_count()) == (c0 + 2, f0 + 2) and eng.assoc_counts() == a0
    eng.detections()
    fresh = pkg.Engine(0)                                        # no scan
    with pytest.raises(pkg.SlamError) as err:
        fresh.detect_scan_fit_dev((0.1, 0.0))
    assert err.value.status == -4 and fresh.detect_fit_count() == 0
    fresh.close()
