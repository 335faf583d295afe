"""tests/_estimate_spec.py — the exact restatement of slam_pf_mean and slam_pf_best that tests/test_gpu_estimates.py holds the
kernels to — against float64 math, with a DERIVED bound, and the proof that every case sits on the edge it names."""
import math

import numpy as np
import pytest

import _estimate_spec as E
import _shard_worker as W

# every n of the GPU test small enough to pin here in a moment; the restatement does not change with n
SIZES = [1, 63, 64, 65, 255, 256, 257, 2047, 2049]
DET_SINCOS_ERR = 2.5e-7          # |det_sincos - libm| on [-20, 20]: tests/test_oracle_pf.py::test_det_math_accuracy
REFS = E.REFS


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def _bounds(x, y, th, ref, pose, r, weighted):
    """The bound, written out.  x, y: every truncation loses less than one unit of 2^-32 m, so does the mean of the truncated
    values (weighted: plus less than one unit for the truncated quotient); half an ulp for the final binary32 rounding; 2^-50
    relative for the float64 arithmetic on either side.
    Heading: a term sin / cos(th_i - ref) is off by at most the stated error of det_sincos, less than one unit of 2^-30 for its
    truncation and half an ulp of the binary32 difference th_i - ref; the mean vector therefore moves by at most sqrt(2) times
    that (weighted: plus 2^-30 per component for the truncated quotients), and a vector of length r moved by e turns by at
    most asin(e / r) <= e / (r - e); half an ulp for the final rounding."""
    units = 2 if weighted else 1
    bx = units * 2.0 ** -32 + 0.5 * _ulp32(pose[0]) + 2.0 ** -50 * float(np.abs(x).max())
    by = units * 2.0 ** -32 + 0.5 * _ulp32(pose[1]) + 2.0 ** -50 * float(np.abs(y).max())
    dmax = float(np.abs(th.astype(np.float64) - ref).max())
    term = DET_SINCOS_ERR + 2.0 ** -30 + 0.5 * _ulp32(dmax)
    e = math.sqrt(2.0) * (term + (2.0 ** -30 if weighted else 0.0))
    bth = e / (r - e) + 0.5 * _ulp32(pose[2]) + 1e-12
    return bx, by, bth


@pytest.mark.parametrize("name", ["plain", "straddle_pi", "negative", "large"])
@pytest.mark.parametrize("n", SIZES)
def test_mean_spec_against_float64(orc, name, n):
    x, y, th = E.edge_population(name, n)
    rng = np.random.default_rng(n)
    idx = np.sort(rng.integers(0, n, n)).astype(np.int32)          # a pending gather: repeats and gaps
    w16 = [int(v) for v in rng.integers(0, 2 ** 16 + 1, n)]
    w16[0] = 2 ** 16                                                # the heaviest particle of a frame always has 2^16
    for ref in REFS[name]:
        for gather in (None, idx):
            for w in (None, w16):
                pose, sums = E.mean_spec(x, y, th, gather, ref, n, w)
                g = slice(None) if gather is None else gather
                mx, my, mth, r = E.f64_means(x[g], y[g], th[g], ref, w)
                assert r > 0.5                                       # the populations are concentrated: the bound means something
                bx, by, bth = _bounds(x[g], y[g], th[g], float(np.float32(ref)), pose, r, w is not None)
                assert abs(float(pose[0]) - mx) <= bx and abs(float(pose[1]) - my) <= by, (name, n, ref)
                assert abs(float(pose[2]) - mth) <= bth, (name, n, ref, float(pose[2]), mth, bth)
                assert len(sums) == (4 if w is None else 5)


@pytest.mark.parametrize("n", [65, 2049, 200000])
def test_cases_sit_on_their_edges(orc, n):
    # straddling +-pi: the arithmetic mean of the headings is more than 1 rad away from the circular one
    x, y, th = E.edge_population("straddle_pi", n)
    circ = E.f64_means(x, y, th, math.pi)[2]
    assert abs(float(th.astype(np.float64).mean()) - circ) > 1.0
    # negative coordinates: truncation and floor give different sums
    x, y, th = E.edge_population("negative", n)
    assert (x < 0).all() and (y < 0).all()
    assert sum(E.trunc_fixed(x, 32)) != sum(E.floor_fixed(x, 32)) and sum(E.trunc_fixed(y, 32)) != sum(E.floor_fixed(y, 32))
    s, _ = orc.det_sincos(th)                                              # ref = 0: every sine is negative and small
    assert (s < 0).all()
    assert sum(E.trunc_fixed(s, 30)) != sum(E.floor_fixed(s, 30))
    # large coordinates: inside the limit of the unweighted 64-bit sum, n * max|x| < 2^31 m (slam_hip.h), and close to it
    x, y, th = E.edge_population("large", n)
    for a in (x, y):
        assert 0.9 * 2 ** 31 < n * float(np.abs(a).max()) < 2 ** 31
        assert abs(sum(E.trunc_fixed(a, 32))) < 2 ** 63 and abs(sum(E.trunc_fixed(a, 32))) > 2 ** 62


def test_best_spec():
    x, y, th = (np.arange(8, dtype=np.float32) + k for k in (10, 20, 30))
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    lw = np.array([-3, 2, -1, 2, 2, -inf, -inf, 0], np.float32)
    assert (lw == lw.max()).sum() >= 2                                      # tied maxima: the lowest index wins
    pose, v, i = E.best_spec(lw, x, y, th, first_id=100)
    assert (i, float(v)) == (101, 2.0) and pose.tolist() == [11.0, 21.0, 31.0]
    lw[1] = nan                                                             # NaN never wins, wherever it stands
    assert E.best_spec(lw, x, y, th)[2] == 3
    lw[:] = [nan, 5, nan, 5, 1, 1, 1, 1]
    assert E.best_spec(lw, x, y, th)[2] == 1
    for all_low in ([-inf] * 8, [nan] * 8, [nan, -inf, nan, -inf, -inf, nan, nan, -inf]):   # nothing to choose from
        pose, v, i = E.best_spec(np.array(all_low, np.float32), x, y, th, first_id=7)
        assert i == 7 and v == -inf and pose.tolist() == [10.0, 20.0, 30.0]
    assert E.best_spec(np.array([-inf, -inf, -7.5, -inf], np.float32), x, y, th)[2] == 2   # a -inf tail and head


def test_weighted_sums_cannot_overflow_their_limbs():
    """slam_hip.h: |x|, |y| <= 1000 m (indeed 1024) at n_total = 2^23.  The kernel adds, per value V, w16 * (V >> 21) and
    w16 * (V & 0x1fffff) into signed 64-bit sums; the host joins them as hi * 2^21 + lo in 128 bits."""
    n, w_max = 2 ** 23, 2 ** 16                       # quantise() clamps a weight at 2^32, so w16 <= 2^16
    v_max = 1024 * 2 ** 32                            # |X|, |Y| (|S|, |C| <= 2^30 are far smaller)
    assert 1000 * 2 ** 32 < v_max
    hi, lo = v_max >> 21, 0x1fffff
    assert n * w_max * hi < 2 ** 63 and n * w_max * lo < 2 ** 63 and n * w_max < 2 ** 63
    assert n * w_max * v_max >= 2 ** 64               # ... whereas the unsplit product does not fit: hence the limbs
    for v in (-v_max, -v_max + 12345, -1, 0, 1, 2 ** 21, v_max - 1, v_max):   # the split is exact for either sign
        assert (v >> 21) * 2 ** 21 + (v & 0x1fffff) == v and abs(v >> 21) <= hi
    # the plain sum: n_total * max|x| < 2^31 m, i.e. 256 m at 2^23 particles
    assert n * 255 * 2 ** 32 < 2 ** 63 <= n * 256 * 2 ** 32


@pytest.mark.parametrize("n", sorted(E.GATED_SCENARIOS))
def test_gated_scenarios_hold_what_they_promise(orc, n):
    """By the specification's own verdicts each scenario of the GPU test has two kept frames in a row, a resampled frame behind a
    kept one, its set_poses / reset behind a kept frame, and a kept frame whose weighted and plain means differ by more than
    16 binary32 ulps in x or y: a mean that ignores the weights cannot pass the GPU test."""
    sc = E.GATED_SCENARIOS[n]
    meta, edt, bx, by, lm = W.make_world(L=1)
    x, y, th, _ = W.init_state(n, 0, lm[:0])
    ev = E.gated_oracle_run((meta, edt, bx, by), x, y, th, n, **sc)
    kinds = "".join("|" if e[1] is None else "R" if e[1] else "k" for e in ev)
    print(n, kinds)
    assert "kk" in kinds and "kR" in kinds and "k|" in kinds
    ulps = [max(abs(int(e[2][:2].view(np.uint32)[k]) - int(e[3][:2].view(np.uint32)[k])) for k in (0, 1))
            for e in ev if e[1] is False]
    assert max(ulps) > 16, ulps
