"""slam_ekf_update_aniso_dev (the landmark update with a 2x2 sensor-frame measurement covariance, csrc/ekf_kernels.hip under EkfNoiseAniso)
against its specification tests/_aniso_spec.py, bit for bit: rows, log-likelihoods, unobserved landmarks, and the columns
below L whatever the padding holds.  Every (n, L) runs the three forms x four observation patterns x two covariances."""
import numpy as np
import pytest
import torch

import _aniso_spec as A
import _f64_pf as F
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 3, 65, 1000)
LS = (1, 31, 128, 129, 257, 500)
COVS = {"correlated": (0.02, 0.012, 0.015), "axis-aligned 1e4:1": (4e-6, 0.0, 4e-2)}
PATTERNS = ("all", "third", "none", "last")
FORMS = ("gather", "identity", "inplace")


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


def make_case(n, L, Lp, seed):
    """Poses with headings beyond +-pi, priors whose condition number runs up to 1e4 (by landmark), 10 % first sightings, prior
    means near the point each particle observes; the padding [L, Lp) holds junk — negative P_xx (the first-sighting marker),
    large values and NaN."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-50, 50, n).astype(np.float32)
    y = rng.uniform(-50, 50, n).astype(np.float32)
    th = rng.uniform(-12.0, 12.0, n).astype(np.float32)
    rows = np.empty((n, 5, Lp), np.float32)
    for j, kappa in enumerate((1.0, 1e2, 1e4)):
        cols = np.arange(j, L, 3)
        if len(cols):
            pxx, pxy, pyy = F.random_priors(rng, (n, len(cols)), 0.02, 10.0 ** rng.uniform(-2, 2), kappa)
            rows[:, 2, cols], rows[:, 3, cols], rows[:, 4, cols] = pxx, pxy, pyy
    zx = rng.uniform(-20, 20, L).astype(np.float32)
    zy = rng.uniform(-20, 20, L).astype(np.float32)
    wx, wy = F.first_sighting(zx[None], zy[None], x[:, None], y[:, None], th[:, None])
    rows[:, 0, :L] = wx + 0.3 * rng.standard_normal((n, L))
    rows[:, 1, :L] = wy + 0.3 * rng.standard_normal((n, L))
    rows[:, 2, :L][rng.random((n, L)) < 0.1] = -1.0
    pad = rng.standard_normal((n, 5, Lp - L)).astype(np.float32) * 1e3
    pad[rng.random(pad.shape) < 0.2] = np.nan
    rows[:, :, L:] = pad
    return (x, y, th), rows, zx, zy


def observed(pattern, L):
    return {"all": np.arange(L), "third": np.arange(0, L, 3), "none": np.arange(0), "last": np.array([L - 1])}[pattern].astype(np.int32)


def run_all(eng, n, L, Lp, seed):
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, seed)
    rng = np.random.default_rng(seed + 1)
    anc = rng.integers(0, n, n).astype(np.int32)   # repeated and out-of-order ancestors
    dx, dy, dth, danc = dev(x), dev(y), dev(th), dev(anc)
    d_in = dev(rows)
    d_ll = torch.empty(n, device=DEV)
    checked = 0
    for pattern in PATTERNS:
        ids = observed(pattern, L)
        eng.obs_upload(ids, zx[ids], zy[ids], L)
        for name, cov in COVS.items():
            for form in FORMS:
                label = f"n={n} L={L} Lp={Lp} {form} obs={pattern} Q={name}"
                a = anc if form == "gather" else None
                want, want_ll = A.update(rows, x, y, th, a, ids, zx[ids], zy[ids], cov, L=L, in_place=form == "inplace")
                if form == "inplace":
                    d_out = d_in.clone()
                    eng.ekf_update_aniso_dev(d_out, d_out, 5 * Lp, Lp, L, dx, dy, dth, None, n, cov, d_ll)
                else:
                    d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
                    eng.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, dx, dy, dth, danc if a is not None else None, n, cov, d_ll)
                got, got_ll = host(d_out), host(d_ll)
                assert np.array_equal(bits(got[:, :, :L]), bits(want[:, :, :L])), f"{label}: rows"
                assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: log-likelihoods"
                if form == "inplace":   # in place nothing but the observed landmarks is touched, the padding included
                    rest = np.setdiff1d(np.arange(Lp), ids)
                    assert np.array_equal(bits(got[:, :, rest]), bits(rows[:, :, rest])), f"{label}: unobserved columns changed"
                checked += 1
    assert np.array_equal(bits(host(d_in)), bits(rows)), "the source rows of an out-of-place update changed"
    return checked


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_update_equals_the_spec(eng, n, L):
    Lp = (L + 31) // 32 * 32
    assert run_all(eng, n, L, Lp, 1000 * n + L) == len(PATTERNS) * len(COVS) * len(FORMS)


@pytest.mark.parametrize("n,L,Lp", [(65, 257, 384), (3, 500, 512)])
def test_plane_stride_a_multiple_of_128(eng, n, L, Lp):
    """... where whole batches run unpredicated over the padding (the fast path of the row walk)."""
    run_all(eng, n, L, Lp, 77)


def test_padding_does_not_reach_the_columns_below_L(eng):
    (x, y, th), rows, zx, zy = make_case(65, 129, 160, 5)
    other = rows.copy()
    other[:, :, 129:] = 0.0
    ids = observed("third", 129)
    eng.obs_upload(ids, zx[ids], zy[ids], 129)
    out = []
    dx, dy, dth = dev(x), dev(y), dev(th)
    for r in (rows, other):
        d_in, d_out, d_ll = dev(r), torch.empty((65, 5, 160), device=DEV), torch.empty(65, device=DEV)
        eng.ekf_update_aniso_dev(d_in, d_out, 5 * 160, 160, 129, dx, dy, dth, None, 65, COVS["correlated"], d_ll)
        out.append((host(d_out)[:, :, :129], host(d_ll)))
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1]))


def test_loglikelihoods_stay_in_the_engine(eng):
    """slam_logweight_ekf_dev picks up what the update left: with a zero score, logw = loglik - 0."""
    n, L, Lp = 65, 31, 32
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 9)
    ids = observed("all", L)
    eng.obs_upload(ids, zx, zy, L)
    d_in, d_out, dx, dy, dth = dev(rows), torch.empty((n, 5, Lp), device=DEV), dev(x), dev(y), dev(th)
    logw, score = torch.empty(n, device=DEV), torch.zeros(n, device=DEV)
    torch.cuda.synchronize()
    eng.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, dx, dy, dth, None, n, COVS["correlated"], None)
    eng.logweight_ekf_dev(score, 1.0, n, logw, None)
    eng.sync()
    _, want_ll = A.update(rows, x, y, th, None, ids, zx, zy, COVS["correlated"], L=L)
    assert np.array_equal(bits(host(logw)), bits(want_ll - np.float32(0.0)))


BAD = [(float("nan"), 0.0, 1.0), (1.0, float("nan"), 1.0), (1.0, 0.0, float("inf")), (0.0, 0.0, 1.0), (-1.0, 0.0, 1.0), (1.0, 0.0, 0.0),
       (1.0, 0.0, -2.0), (1.0, 1.0, 1.0), (1.0, -1.5, 1.0), (1e-30, 0.0, 1e-30)]


def test_rejected_covariances_and_counters(eng):
    """A Q that is not finite, not positive definite, or whose float32 determinant is not positive is refused with
    SLAM_ERR_INVALID_ARG and nothing is launched; the engine goes on.  Launches count in slam_ekf_aniso_count alone."""
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    (x, y, th), rows, zx, zy = make_case(n, L, Lp, 3)
    ids = observed("all", L)
    eng.obs_upload(ids, zx, zy, L)
    d_in, d_out, d_ll = dev(rows), torch.full((n, 5, Lp), 7.0, device=DEV), torch.empty(n, device=DEV)
    args = (5 * Lp, Lp, L, dev(x), dev(y), dev(th), None, n)
    c0, f0, i0 = eng.ekf_aniso_count(), eng.ekf_form_counts(), eng.ekf_inplace_form_counts()
    for q in BAD:
        assert not A.valid_cov(q), q
        with pytest.raises(pkg.SlamError) as err:
            eng.ekf_update_aniso_dev(d_in, d_out, *args, q, d_ll)
        assert err.value.status == -2 and "meas_cov must be finite" in str(err.value), (q, str(err.value))
    assert eng.ekf_aniso_count() == c0 and np.all(host(d_out) == 7.0)
    cov = COVS["axis-aligned 1e4:1"]
    eng.ekf_update_aniso_dev(d_in, d_out, *args, cov, d_ll)
    d_same = d_in.clone()
    eng.ekf_update_aniso_dev(d_same, d_same, *args, cov, d_ll)
    want, want_ll = A.update(rows, x, y, th, None, ids, zx, zy, cov, L=L)
    assert np.array_equal(bits(host(d_out)[:, :, :L]), bits(want[:, :, :L])) and np.array_equal(bits(host(d_ll)), bits(want_ll))
    assert eng.ekf_aniso_count() == c0 + 2
    assert eng.ekf_form_counts() == f0 and eng.ekf_inplace_form_counts() == i0
    # the argument checks of slam_ekf_update_dev: a gather in place, a plane stride below L, no observation table for this L
    for bad_call in (lambda: eng.ekf_update_aniso_dev(d_same, d_same, 5 * Lp, Lp, L, *args[3:6], dev(np.zeros(n, np.int32)), n, cov, None),
                     lambda: eng.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, L - 1, L, *args[3:], cov, None),
                     lambda: eng.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, Lp, L - 1, *args[3:], cov, None)):
        with pytest.raises(pkg.SlamError):
            bad_call()
