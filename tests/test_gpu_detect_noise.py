"""slam_detect_scan_noise_dev (the detector's noise model, csrc/detect_kernels.hip: kNoise) against its specification
tests/_detect_noise_spec.py: detections, their covariances (slam_detections_get_cov_host), ndet and all six stats words are equal
bit for bit on the pole fields of the detector's own tests, with and without a fit and wrap, with more than 64 accepted segments
and with none, and under a model whose determinants cancel; without a model the entry point is slam_detect_scan_fit_dev; the
counters and the argument checks."""
import numpy as np
import pytest
import torch

import _detect_fit_spec as DF
import _detect_noise_spec as DN
import _detect_scenes as S
from __graft_entry__ import load_package
from conftest import bits
from test_gpu_detect_fit import DEV, GUARD, dev, eng, host   # noqa: F401 - eng is a fixture

pytestmark = pytest.mark.gpu
PS = (0, 1, 63, 64, 65, 257, 360, 4096)
MODELS = ((1e-4, 1.5625e-4, 1e-4), (1e-12, 1.0, 0.0))     # a lidar's; one whose determinants cancel off the axes


def check(eng, bx, by, kw, fit, noise, label):
    """One launch against the spec -> the spec's (zx, zy, q, ndet, stats)."""
    want = DN.detect_noise(bx, by, fit, noise, **kw)
    eng.scan_upload(bx, by)
    d = torch.full((14,), GUARD, dtype=torch.int32, device=DEV)   # guard words before and behind the six stats
    c0 = (eng.detect_count(), eng.detect_fit_count(), eng.detect_noise_count())
    eng.detect_scan_noise_dev(noise, fit, d_stats=d[4:10], **kw)
    zx, zy, ndet = eng.detections(full=True)
    q = eng.detections_cov()
    st = host(d)
    assert (eng.detect_count(), eng.detect_fit_count(), eng.detect_noise_count()) == (c0[0] + 1, c0[1] + (fit is not None), c0[2] + 1)
    assert ndet == want[3], f"{label}: ndet {ndet} != {want[3]}"
    assert np.array_equal(st[4:10], want[4]), f"{label}: stats {st[4:10].tolist()} != {want[4].tolist()}"
    assert np.all(st[:4] == GUARD) and np.all(st[10:] == GUARD), f"{label}: written beside the stats"
    assert np.array_equal(bits(zx), bits(want[0])) and np.array_equal(bits(zy), bits(want[1])), f"{label}: detections"
    for g, w in zip(q, want[2]):
        assert len(g) == ndet and np.array_equal(bits(g), bits(w[:ndet])), f"{label}: covariances"
    return want


@pytest.mark.parametrize("P", PS)
def test_pole_fields(eng, P):
    accepted = dropped = 0
    for wrap in (1, 0):
        for fit in (None, (0.1, 0.0), (0.3, 0.0)):
            for noise in MODELS:
                bx, by, kw = S.pole_field(P, 100 + P)
                want = check(eng, bx, by, dict(kw, wrap=wrap), fit, noise, f"P={P} wrap={wrap} fit={fit} noise={noise}")
                accepted += int(want[4][1])
                dropped += int(want[4][4])
    if P >= 257:
        assert accepted > 0 and dropped > 0
    if P == 4096:                       # more than 64 accepted: the cap behind the noise rule
        want = check(eng, bx, by, kw, (0.3, 0.0), MODELS[0], "the cap")
        assert want[4][1] > 64 and want[3] == 64
        want = check(eng, bx, by, kw, (0.3, 0.0), (1e-5, 1.0, 0.0), "the cap behind the drops")   # (the spec: 85 dropped, 95 left)
        assert want[4][4] > 0 and want[4][1] > 64 and want[3] == 64


def test_a_scan_with_no_detection_and_one_on_the_sensor(eng):
    a = -np.pi + 2 * np.pi * np.arange(360) / 360
    bx, by = (5 * np.cos(a)).astype(np.float32), (5 * np.sin(a)).astype(np.float32)
    kw = dict(S.pole_field(360, 1)[2])
    want = check(eng, bx, by, kw, None, MODELS[0], "a round wall")
    assert want[3] == 0 and want[4][1] == 0
    # three points whose centroid is the sensor itself: r2 == 0, dropped by the noise rule and counted
    bx[100:103], by[100:103] = [0.01, -0.02, 0.01], [0.0, 0.0, 0.0]
    want = check(eng, bx, by, kw, None, MODELS[0], "a centroid on the sensor")
    assert want[3] == 0 and want[4][4] == 1


def test_without_a_model_it_is_the_fitted_detector(eng):
    bx, by, kw = S.pole_field(360, 460)
    for fit in (None, (0.2, 0.0)):
        eng.scan_upload(bx, by)
        d = torch.full((14,), GUARD, dtype=torch.int32, device=DEV)
        eng.detect_scan_fit_dev(fit, d_stats=d[4:8], **kw)
        a = eng.detections(full=True), host(d)
        d = torch.full((14,), GUARD, dtype=torch.int32, device=DEV)
        c0 = (eng.detect_count(), eng.detect_fit_count(), eng.detect_noise_count())
        eng.detect_scan_noise_dev(None, fit, d_stats=d[4:10], **kw)
        b = eng.detections(full=True), host(d)
        assert (eng.detect_count(), eng.detect_fit_count(), eng.detect_noise_count()) == (c0[0] + 1, c0[1] + (fit is not None), c0[2])
        assert np.array_equal(bits(a[0][0]), bits(b[0][0])) and np.array_equal(bits(a[0][1]), bits(b[0][1])) and a[0][2] == b[0][2]
        assert np.array_equal(a[1], b[1])                                # four stats words, the guards behind them untouched
        with pytest.raises(load_package().SlamError) as err:            # ... and its detections carry no covariance
            eng.detections_cov()
        assert err.value.status == -4


def test_argument_checks(eng):
    pkg = load_package()
    bx, by, kw = S.pole_field(360, 460)
    eng.scan_upload(bx, by)
    eng.detect_scan_noise_dev(MODELS[0], None, **kw)
    before = eng.detections(full=True), eng.detections_cov()
    c0 = (eng.detect_count(), eng.detect_noise_count())
    for bad in ((0.0, 1.0, 0.0), (-1.0, 1.0, 0.0), (1.0, 0.0, 0.0), (1.0, -1.0, 2.0), (float("nan"), 1.0, 0.0), (1.0, float("inf"), 0.0),
                (1.0, 1.0, float("nan"))):
        assert not DN.noise_ok(bad)
        with pytest.raises(pkg.SlamError) as err:
            eng.detect_scan_noise_dev(bad, None, **kw)
        assert err.value.status == -2 and "noise model" in str(err.value), (bad, str(err.value))
    with pytest.raises(pkg.SlamError) as err:
        eng.detect_scan_noise_dev(MODELS[0], (0.0, 0.0), **kw)
    assert err.value.status == -2
    after = eng.detections(full=True), eng.detections_cov()
    assert (eng.detect_count(), eng.detect_noise_count()) == c0           # nothing was launched, nothing changed
    assert all(np.array_equal(bits(np.asarray(a)), bits(np.asarray(b))) for a, b in zip(before[0] + before[1], after[0] + after[1]))
