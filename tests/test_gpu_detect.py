"""slam_detect_scan_dev (the landmark detector, csrc/detect_kernels.hip) against its specification tests/_detect_spec.py: zx, zy,
ndet and the stats are equal bit for bit at every scan size around the kernel's lane, wavefront and round boundaries, with and
without wrap, on the hand-made scans of tests/_detect_scenes.py and on random pole fields; nothing is written beside the stats;
the pending count reaches the association; slam_detections_get_host; a later upload wins; the argument checks and the counter."""
import numpy as np
import pytest
import torch

import _assoc_spec as A
import _detect_scenes as S
import _detect_spec as D
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_aniso import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096)
SCENES = S.scenarios()
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


def check(eng, bx, by, kw, label):
    """One launch against the spec -> the spec's (zx, zy, ndet, stats)."""
    want = D.detect(bx, by, **kw)
    eng.scan_upload(bx, by)
    d = torch.full((12,), GUARD, dtype=torch.int32, device=DEV)   # guard words before and behind the four stats
    eng.detect_scan_dev(d_stats=d[4:8], **kw)
    zx, zy, ndet = eng.detections(full=True)
    st = host(d)
    print(f"{label}: P={len(bx)} stats={st[4:8].tolist()} want={want[3].tolist()}")
    assert ndet == want[2], f"{label}: ndet {ndet} != {want[2]}"
    assert np.array_equal(st[4:8], want[3]), f"{label}: stats {st[4:8].tolist()} != {want[3].tolist()}"
    assert np.all(st[:4] == GUARD) and np.all(st[8:] == GUARD), f"{label}: written beside the stats"
    assert np.array_equal(bits(zx), bits(want[0])) and np.array_equal(bits(zy), bits(want[1])), f"{label}: detections"
    assert not bits(zx[ndet:]).any() and not bits(zy[ndet:]).any(), f"{label}: entries behind ndet"
    return want


@pytest.mark.parametrize("P", PS)
def test_pole_fields(eng, P):
    accepted = 0
    for wrap in (1, 0):
        bx, by, kw = S.pole_field(P, 100 + P)
        want = check(eng, bx, by, dict(kw, wrap=wrap), f"P={P} wrap={wrap}")
        accepted += int(want[3][1])
    if P >= 63:
        assert accepted > 0
    if P >= 4095:
        assert want[3][1] > 64          # the cap: the first 64 by start index


@pytest.mark.parametrize("name", sorted(SCENES))
def test_scenarios(eng, name):
    bx, by, kw, _ = SCENES[name]
    check(eng, bx, by, kw, name)


@pytest.mark.parametrize("P", (256, 1024, 1088, 4096))
def test_segments_across_every_word_boundary(eng, P):
    """A pole of six points across every multiple of 64 — the last lane of one wavefront and the first of the next, of one round
    of the workgroup and the next — and, cyclically, across the end of the scan."""
    R = 0.1 * P / (2 * np.pi)
    r = np.full(P, R)
    for c in range(0, P, 64):
        r[np.arange(c - 3, c + 3) % P] = 0.7 * R
    a = -np.pi + 2 * np.pi * np.arange(P) / P
    bx, by = (r * np.cos(a)).astype(np.float32), (r * np.sin(a)).astype(np.float32)
    kw = dict(D.DEFAULTS, max_range=1000.0)
    want = check(eng, bx, by, kw, f"boundaries P={P}")
    assert want[3][1] == P // 64 and want[2] == min(P // 64, 64)
    want = check(eng, bx, by, dict(kw, wrap=0), f"boundaries P={P} wrap=0")
    assert want[3][1] == P // 64 - 1


def _associate(eng, case, n, L, Lp):
    poses, rows = case
    d_assoc = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
    eng.associate_dev(dev(rows), 5 * Lp, Lp, L, dev(poses[0]), dev(poses[1]), dev(poses[2]), None, n, 0.02, 9.21, 50.0, 1, d_assoc, Lp, d_st)
    return host(d_assoc), host(d_st)


@pytest.mark.parametrize("scene", ["field", "many", "empty"])
def test_pending_count_reaches_the_association(eng, scene):
    """slam_associate_dev right after slam_detect_scan_dev = after slam_detections_upload_host of the spec's output."""
    n, L, Lp = 65, 100, 128
    poses, rows, _, _ = make_case(n, L, Lp, 21)
    bx, by, kw = S.pole_field(360, 9) if scene == "field" else SCENES[scene][:3]
    zx, zy, k, _ = D.detect(bx, by, **kw)
    assert k == {"field": k, "many": 64, "empty": 0}[scene] and (scene != "field" or 3 < k < 64)
    eng.scan_upload(bx, by)
    eng.detect_scan_dev(**kw)
    got = _associate(eng, (poses, rows), n, L, Lp)
    eng.detections_upload(zx[:k], zy[:k])
    want = _associate(eng, (poses, rows), n, L, Lp)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    spec = A.associate(rows, *poses, None, zx[:k], zy[:k], 0.02, 9.21, 50.0, 1, L=L, assoc_stride=Lp)
    assert np.array_equal(got[0], spec[0]) and np.array_equal(got[1], spec[1])
    assert int(got[1][:, :2].sum()) > 0 or k == 0


def test_get_host_and_a_later_upload_wins(eng):
    bx, by, kw = S.pole_field(360, 9)
    want = D.detect(bx, by, **kw)
    eng.scan_upload(bx, by)
    eng.detect_scan_dev(**kw)
    zx, zy = eng.detections()
    assert len(zx) == want[2] and np.array_equal(bits(zx), bits(want[0][:want[2]])) and np.array_equal(bits(zy), bits(want[1][:want[2]]))
    # an upload behind a detector launch whose count nobody picked up: the upload is what counts
    eng.detect_scan_dev(**kw)
    mine = np.array([1.5, -2.5], np.float32), np.array([0.25, 4.0], np.float32)
    eng.detections_upload(*mine)
    zx, zy, k = eng.detections(full=True)
    assert k == 2 and np.array_equal(zx[:2], mine[0]) and np.array_equal(zy[:2], mine[1]) and not zx[2:].any() and not zy[2:].any()
    n, L, Lp = 3, 8, 32
    poses, rows, _, _ = make_case(n, L, Lp, 5)
    rows[:, 2] = -1.0                                    # empty maps: every detection is new
    got = _associate(eng, (poses, rows), n, L, Lp)
    assert np.all(got[1] == [0, 2, 0])
    # ... and device arrays handed over likewise
    d = dev(np.array([3.0, 4.0, 5.0], np.float32))
    eng.detect_scan_dev(**kw)
    eng.detections_set_dev(d, d, 3)
    zx, zy = eng.detections()
    assert zx.tolist() == [3.0, 4.0, 5.0] and zy.tolist() == [3.0, 4.0, 5.0]
    eng.detections_upload(np.zeros(0, np.float32), np.zeros(0, np.float32))


def test_argument_checks_and_the_counter(eng):
    pkg = load_package()
    bx, by, kw = S.pole_field(64, 1)
    eng.scan_upload(bx, by)
    c0, a0, e0 = eng.detect_count(), eng.assoc_counts(), eng.evidence_counts()
    for bad in (dict(jump=0.0), dict(jump=float("nan")), dict(jump=float("inf")), dict(guard=0.2), dict(guard=float("nan")),
                dict(max_width=0.0), dict(max_width=float("inf")), dict(max_range=-1.0), dict(max_range=float("nan")),
                dict(min_points=0), dict(min_points=5, max_points=4), dict(max_points=65), dict(wrap=2), dict(wrap=-1)):
        assert not D.params_ok(D.params(**bad))
        with pytest.raises(pkg.SlamError) as err:
            eng.detect_scan_dev(**bad)
        assert err.value.status == -2, bad
    assert eng.lib.slam_detect_scan_dev(eng.h, None, None) == -2
    assert eng.detect_count() == c0
    p = pkg.DetectParams.default()
    assert (round(p.jump, 6), p.guard, p.max_width, p.max_range, p.min_points, p.max_points, p.wrap) == (0.3, 1.0, 0.5, 20.0, 3, 40, 1)
    eng.detect_scan_dev(p)                               # d_stats may be NULL
    eng.detect_scan_dev(**kw)
    assert eng.detect_count() == c0 + 2 and eng.assoc_counts() == a0 and eng.evidence_counts() == e0
    eng.detections()
    fresh = pkg.Engine(0)                                # no scan, no detections
    for call in (fresh.detect_scan_dev, fresh.detections):
        with pytest.raises(pkg.SlamError) as err:
            call()
        assert err.value.status == -4
    assert fresh.detect_count() == 0
    fresh.close()


def test_bracketed_as_pages(eng):
    bx, by, kw = S.pole_field(360, 2)
    eng.scan_upload(bx, by)
    eng.profile_enable(eng.PROF_PAGES)
    eng.profile_read(eng.PROF_PAGES)
    eng.detect_scan_dev(**kw)
    ms, launches = eng.profile_read(eng.PROF_PAGES)
    eng.profile_enable()
    eng.detections()
    assert launches == 1 and 0.0 < ms < 50.0
