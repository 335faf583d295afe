"""The particle-filter SPECIFICATION (oracle/slam_oracle_pf.c, rows A9-A12) against an independent float64 reference
(tests/_f64_pf.py: Philox in numpy integers, Box-Muller in float64, the sensor-frame Joseph-form EKF, float64 weights and
systematic resampling) — not bit for bit, but within forward-error bounds.

Every HIP kernel is pinned bit for bit to the specification elsewhere, and the specification restates the kernels'
world-frame algebra (csrc/ekf_math.h), so a numerically unsound formula would pass those tests on both sides.  These
tests judge the arithmetic itself.  The bounds (u = 2^-24, written out in _f64_pf.update_errors and resample_check) are
    motion      |x - x_64| <= 4 u (|x_src| + |dp|) + 40 u sigma R,  R = sqrt(-2 log 2^-24) (the largest Box-Muller radius)
    mean        |mu' - mu'_64| <= 4 u (|t| + |mu| + |d| (1 + kappa(S) q / lambda_min(S))) + 4 (SINCOS_ABS + u) |z|
    covariance  max_ij |P'_ij - P'_64,ij| <= 4 u ((kappa(S) + 2) lambda_max(P') + q (P_xx P_yy + P_xy^2) / det S)
    log-lik     |ll - ll_64| <= 8 u (kappa(S) (1 + m) + |log det S| + 1) + 2 sqrt(m / lambda_min(S)) e_d  per landmark,
                plus (ceil(L / 128) + 7) u sum |ll| for the summation over landmarks
    log-weight  |logw - logw_64| <= the log-likelihood's bound + 2 u (|ll| + |gain score|)
and the resample's ancestors may differ from the float64 ones only at comb teeth within the weights' quantisation error
of a CDF boundary (never by more than one offspring per particle).  The stored posterior covariance must be positive
definite, exactly (in float64, from the float32 values).  The old posterior, P' = P - W P and mu' = mu + W d with the gain
W -> I, broke the covariance bound by 10 .. 10^7 at P / q >= 1e4 and on elongated priors (kappa(P) >= 1e2 at
P / q = 1e2), with non-positive-definite posteriors from P / q = 1e4, kappa 1e4.
"""
import numpy as np
import pytest

import _f64_pf as F

U = F.U


def test_philox_known_answers():
    """Random123 kat_vectors, philox4x32-10 (the numpy implementation of the reference)."""
    def one(ctr, key):
        return [hex(int(v)) for v in F.philox4x32_10([np.uint64(c) for c in ctr], key)]
    assert one([0, 0, 0, 0], (0, 0)) == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    assert one([0xFFFFFFFF] * 4, (0xFFFFFFFF, 0xFFFFFFFF)) == ["0x408f276d", "0x41c83b0e", "0xa20bc7c6", "0x6d5451fd"]
    assert one([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], (0xA4093822, 0x299F31D0)) == [
        "0xd16cfe09", "0x94fdcceb", "0x5001e420", "0x24126ea1"]


@pytest.mark.parametrize("n,first_id,pose_max,sigma", [(4096, 0, 1.0, (0.05, 0.05, 0.01)),
                                                       (65536, 1 << 33, 1e3, (1.0, 2.0, 0.5)),
                                                       (65536, 12345, 1e3, (1e-3, 7.7, 123.456))])
def test_motion_sample_against_float64(orc, n, first_id, pose_max, sigma):
    rng = np.random.default_rng(n + first_id)
    m = n + 17
    src = [rng.uniform(-pose_max, pose_max, m).astype(np.float32) for _ in range(3)]
    anc = np.sort(rng.integers(0, m, n)).astype(np.int32)
    dp = [0.004, -0.001, 0.0006]
    got = orc.motion_sample(*src, anc, n, first_id, dp, sigma, 77, 5)
    r = F.motion_errors(got, src, anc, dp, sigma, first_id, 77, 5)
    print(f"motion n={n}: max error / bound {r.max():.3g}")
    assert r.max() <= 1.0


def _run_spec(orc, rows, pose, ids, zx, zy, q):
    out, ll = orc.ekf_update(rows, *pose, None, np.asarray(ids, np.int32), zx, zy, np.float32(q))
    return out, ll


@pytest.mark.parametrize("q,ratio,kappa", F.GRID, ids=[f"q{q:g}-Pq{r:g}-k{k:g}" for q, r, k in F.GRID])
def test_ekf_regime_grid(orc, q, ratio, kappa):
    """The whole grid: q in {1e-8, 1e-4, 1e-2}, P / q in {1e-4 .. 1e8}, kappa(P) in {1, 1e2, 1e4} at random orientations,
    |pose| and |theta| up to 1e3, landmarks up to 1e3 m away; 512 particles x 96 landmarks, every landmark observed."""
    rng = np.random.default_rng(int(np.log10(q) * 100 + np.log10(ratio) * 10 + np.log10(kappa)) & 0xFFFF)
    pose, rows, zx, zy = F.regime_frame(rng, 512, 96, q, ratio, kappa)
    ids = np.arange(96)
    out, ll = _run_spec(orc, rows, pose, ids, zx, zy, q)
    F.check_frame(rows, out, ll, pose, ids, zx, zy, q, f"q={q:g} P/q={ratio:g} kappa={kappa:g}")


AT_SIZE = [(1e-2, 1e4, 1e4, 0), (1e-8, 1e8, 1.0, 0), (1e-4, 1e2, 1e2, 0), (1e-2, 1.0, 1.0, 0), (1e-2, 1e2, 1.0, 3)]


@pytest.mark.parametrize("q,ratio,kappa,huge", AT_SIZE, ids=[f"q{a:g}-Pq{b:g}-k{c:g}-h{d}" for a, b, c, d in AT_SIZE])
def test_ekf_at_size(orc, q, ratio, kappa, huge):
    """4 096 particles x 500 landmarks: observations in shuffled order on 7 of 8 landmarks, first sightings mixed in (one
    landmark in 9 never seen by one particle in 5), the rest unobserved.  huge = 3: ~1e10 m^2 priors on every third
    particle (det (P + q I) beyond 2^61, the device's division fallback), next to ordinary ones."""
    n, L = 4096, 500
    rng = np.random.default_rng(500 + huge)
    pose, rows, zx, zy = F.regime_frame(rng, n, L, q, ratio, kappa, huge_every=huge)
    never = (rng.random((n, L)) < 0.2) & (np.arange(L)[None, :] % 9 == 4)
    rows[:, 2][never] = -1.0
    ids = rng.permutation(L)[: L * 7 // 8]
    out, ll = _run_spec(orc, rows, pose, ids, zx[ids], zy[ids], q)
    F.check_frame(rows, out, ll, pose, ids, zx[ids], zy[ids], q, f"at size q={q:g} P/q={ratio:g} kappa={kappa:g} huge={huge}")


@pytest.mark.parametrize("n", [1, 63, 65, 4096, 65536])
def test_weights_and_resample_against_float64(orc, n):
    """logw = ll - gain score, quantised weights exp(logw - max) 2^32 and the systematic resample, against float64."""
    rng = np.random.default_rng(n)
    ll = (rng.standard_normal(n) * 30 - 500).astype(np.float32)
    score = rng.uniform(0, 200, n).astype(np.float32)
    gain = 0.25
    lw, m = orc.logweight(score, ll, gain)
    lw64 = F.logweights(ll, score, gain)
    b = 2 * U * (np.abs(ll) + np.abs(np.float32(gain) * score.astype(np.float64)))
    assert (np.abs(lw - lw64) <= b).all() and m == lw.max()
    wq, total = orc.quantise_weights(lw, m)
    _, w64 = F.weights(lw)
    e = w64 * (6 * U + 2 * U * np.abs(lw.astype(np.float64) - float(m))) + 1.0
    assert (np.abs(wq.astype(np.float64) - w64) <= e).all() and total == int(wq.sum())
    for frame in (0, 3, 11):
        anc = orc.resample(wq, 99, frame)
        nd, dc = F.resample_check(wq, anc, lw, 99, frame)
        print(f"n={n} frame {frame}: {nd} slots off the float64 resample (all at CDF boundaries), count difference {dc}")
