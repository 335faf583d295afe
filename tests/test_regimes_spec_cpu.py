"""The specifications of the 2x2 noise-form stages ALONE on the regime populations of tests/_regimes.py, and what
test_gpu_regimes.py relies on.  (1) The populations are what they claim — the float32 determinants, as each specification
computes them, counted against ekf_rcp's range — on EXACTLY the cases the GPU test runs (_regimes.CASES: its shapes, its seeds;
test_the_gpu_cases_are_what_they_claim) and on one larger shape.  (2) On that larger shape (n = 130, L = 257, K = 64, every q of
the grid) every specification stays inside the float64 bound the existing CPU tests hold it to (the bound functions are the same
objects: _aniso_bounds, _assoc_aniso_bounds, _merge_bounds, _f64_pf).  (3) What the specifications give on the `edge` population,
where the GPU test compares bits alone.  No GPU.

The localise log-likelihood: test_localise_spec_cpu.py's relative bound (1e-5 |ll|) was stated for unit-scale covariances and
poses of a few metres; on these populations (|pose| 1e3, lambda_min(S) down to 2^-32) the error of the innovation alone,
2 sqrt(m / lambda_min(S)) 4 u (|t| + |mu|), exceeds it by orders of magnitude in float64's own sensitivity (DESIGN.md section 7
states the domain).  The stage adds no arithmetic to the update's likelihood term, so here it is held pair by pair to that
term's own forward-error bound (_regimes.localise_check), which is the stronger statement."""
import numpy as np
import pytest

import _aniso_spec as A
import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _assoc_spec as AI
import _localise_detcov_spec as LD
import _localise_spec as LS
import _merge_spec as M
import _regimes as R
from _aniso_bounds import check, cov_domain
from _assoc_aniso_bounds import cost64

N, L, K = 130, 257, 64
GATE, NEW_GATE, MERGE_GATE = 9.21, 50.0, 9.0
CASES = [(p, q) for p in ("ordinary", "mixed") for q in R.QS] + [("high", R.QS[0]), ("high", R.QS[-1]), ("low", R.Q_LOW)]
IDS = [f"{p}-q{q:.3g}" for p, q in CASES]


def seed_of(pop, q, extra=0):
    return R.POPULATIONS.index(pop) * 1000 + int(-np.log2(q)) * 10 + extra


@pytest.mark.parametrize("pop,q", CASES, ids=IDS)
def test_aniso_update(orc, pop, q):
    for j, (name, cov) in enumerate(R.aniso_covs(q, seed_of(pop, q)).items()):
        pose, rows, zx, zy = R.frame(pop, N, L, q, seed_of(pop, q, j), q_lo=float(name.split("=")[1]) ** -1 * q)
        share = R.census(pop, R.dets_aniso(rows, pose[2], cov), f"{pop} {name}")
        out, ll = A.update(rows, *pose, None, np.arange(L), zx, zy, cov)
        assert np.all(np.isfinite(out[:, :, :L])) and np.all(np.isfinite(ll))
        print(f"{pop} q={q:g} {name}: {share:.3f} of the determinants outside the fast reciprocal's range")
        check(rows[:, :, :L], out[:, :, :L], ll, pose, zx, zy, cov, f"aniso update, {pop} q={q:g} {name}", normal=j == 0,
              domain=cov_domain(rows[:, 2, :L], rows[:, 3, :L], rows[:, 4, :L], cov))


def assoc_inputs(pop, q, form):
    """-> (pose, rows, dx, dy, noise, per-detection triples or the meas_var, the determinants of every pair)."""
    s = seed_of(pop, q, 3 + ("iso", "aniso", "detcov").index(form))
    if form == "iso":
        pose, rows, zx, zy = R.frame(pop, N, L, q, s)
        return pose, rows, *R.detections(zx, zy, K, s), float(np.float32(q)), float(np.float32(q)), R.dets_iso(rows, q)
    if form == "aniso":
        cov = R.aniso_covs(q, s)["kappa(Q)=10000"]
        pose, rows, zx, zy = R.frame(pop, N, L, q, s, q_lo=q * 1e-4)
        return pose, rows, *R.detections(zx, zy, K, s), cov, [cov] * K, R.dets_aniso(rows, pose[2], cov)
    covs = R.detection_covs(K, s, q)
    pose, rows, zx, zy = R.frame(pop, N, L, q, s, q_lo=q * R.DETCOV_Q_LO)
    return pose, rows, *R.detections(zx, zy, K, s), covs, list(zip(*covs)), R.dets_detcov(rows, pose[2], covs)


SPEC = {"iso": AI, "aniso": AA, "detcov": AD}


@pytest.mark.parametrize("form", ("iso", "aniso", "detcov"))
@pytest.mark.parametrize("pop,q", CASES, ids=IDS)
def test_association_and_its_update(orc, pop, q, form):
    pose, rows, dx, dy, noise, per_k, det = assoc_inputs(pop, q, form)
    share = R.census(pop, det, f"{pop} {form}")
    S = SPEC[form]
    assoc, st = S.associate(rows, *pose, None, dx, dy, noise, GATE, NEW_GATE, 1)
    out, ll = S.update(rows, *pose, None, assoc, dx, dy, noise)
    print(f"{pop} q={q:g} {form}: {share:.3f} outside the range; matched {st[:, 0].sum()} created {st[:, 1].sum()} dropped {st[:, 2].sum()}")
    assert st[:, 0].sum() + st[:, 1].sum() > 0 and np.all(np.isfinite(ll))
    R.pairs_check(rows, out, ll, pose, assoc, dx, dy, per_k, L, f"{form} association's update, {pop} q={q:g}")
    if form == "aniso":                                               # the cost itself against the float64 sensor-frame term
        seen, m = AA.cost_matrix(rows, *pose, None, dx, dy, noise)
        m64, bound = cost64(np.where((rows[:, 2:3] < 0), np.float32([0, 0, 1, 0, 1])[None, :, None], rows), *pose, dx, dy, noise)
        ratio = np.where(seen[:, :, None], np.abs(m.astype(np.float64) - m64) / bound, 0.0)
        print(f"{pop} q={q:g}: max |m - m_64| / bound {ratio.max():.3g}")
        assert np.all(np.isfinite(m[seen])) and ratio.max() <= 1.0


@pytest.mark.parametrize("pop,q", CASES, ids=IDS)
def test_merge(pop, q):
    mp, tab, ev = R.merge_case(pop, N, L, L + 31, K, q, seed_of(pop, q, 8))
    R.merge_census(pop, mp, tab, K, L, f"{pop} merge")
    out, ev_out, st = M.merge(mp, tab, K, MERGE_GATE, ev, 200, L=L)
    print(f"{pop} q={q:g}: merged {st[:, 0].sum()} refused {st[:, 1].sum()}")
    assert st[:, 0].sum() > 0
    assert R.merge_check(mp, out, tab, K, L, f"merge, {pop} q={q:g}")["checked"] > 1000


@pytest.mark.parametrize("form", ("iso", "detcov"))
@pytest.mark.parametrize("pop,q", CASES, ids=IDS)
def test_localise(orc, pop, q, form):
    s = seed_of(pop, q, 9)
    if form == "iso":
        Mk, x, y, th, dx, dy = R.known_map_case(pop, N, L, K, q, s)
        noise = per_k = float(np.float32(q))
        det = R.dets_iso(Mk[None], q)
        assoc, st, ll = LS.localise(Mk, x, y, th, dx, dy, noise, GATE, 0.0)
    else:
        Mk, x, y, th, dx, dy = R.known_map_case(pop, N, L, K, q, s, q_lo=q * R.DETCOV_Q_LO)
        noise = R.detection_covs(K, s, q)
        per_k = list(zip(*noise))
        det = R.dets_detcov(np.broadcast_to(Mk, (N,) + Mk.shape), th, noise)
        assoc, st, ll = LD.localise(Mk, x, y, th, dx, dy, noise, GATE, 0.0)
    R.census(pop, det, f"{pop} localise {form}")
    print(f"{pop} q={q:g} {form}: matched {st[:, 0].sum()} of {N * K}")
    assert st[:, 0].sum() > 0 and np.all(np.isfinite(ll))
    R.localise_check(Mk, ll, (x, y, th), assoc, dx, dy, per_k, f"localise {form}, {pop} q={q:g}")


@pytest.mark.parametrize("pop,shape", R.CASES, ids=R.CASE_IDS)
def test_the_gpu_cases_are_what_they_claim(orc, pop, shape):
    """Every input test_gpu_regimes.py builds, by the same functions with the same seeds: all, none, or both kinds within one
    64-lane block."""
    n, L, K = shape
    for j in range(2):
        name, cov, pose, rows, zx, zy, det = R.aniso_case(pop, shape, j)
        R.census(pop, det, f"{pop} aniso {name}")
        assert np.abs(pose[0]).max() <= 1e3 and np.abs(pose[2]).max() <= 2e4 and rows.shape[2] > L
        if n >= 3:
            assert (np.abs(pose[2]) == 2e4).any() and np.isnan(rows[:, :, L:]).any()
    for form in R.FORMS:
        R.census(pop, R.assoc_case(pop, shape, form)[-1], f"{pop} association {form}")
    mp, tab, ev = R.merge_case_of(pop, shape)
    R.merge_census(pop, mp, tab, K, L, f"{pop} merge")
    for form in ("iso", "detcov"):
        R.census(pop, R.localise_case(pop, shape, form)[-1], f"{pop} localise {form}")


def test_the_edge_population(orc):
    """det S in [2^126, 2^128) on the even landmarks (a denormal reciprocal), +inf on the odd ones (a reciprocal of 0): what the
    specifications give there — finite means and log-likelihoods, a NaN covariance where det S overflowed, and such landmarks
    taking detections at a Mahalanobis term of 0."""
    n, L, K, q = 65, 257, 64, 1e-2
    pose, rows, zx, zy = R.frame("edge", n, L, q, 4242 + L, Lp=R.padded(L))
    det = R.dets_iso(rows[:, :, :L], q)
    assert np.isinf(det[:, 1::2]).all() and np.all((det[:, 0::2] >= 2.0 ** 126) & np.isfinite(det[:, 0::2]))
    with np.errstate(all="ignore"):
        idet = np.float32(1.0) / det
    assert np.all(idet[:, 1::2] == 0) and np.all((idet[:, 0::2] > 0) & (idet[:, 0::2] < 2.0 ** -126))
    for name, cov in R.aniso_covs(q, 77).items():
        R.census("edge", R.dets_aniso(rows[:, :, :L], pose[2], cov), name)
        out, ll = A.update(rows, *pose, None, np.arange(L), zx, zy, cov, L=L)
        assert np.all(np.isfinite(out[:, :, 0:L:2])) and np.all(np.isfinite(out[:, :2, :L])) and np.all(np.isfinite(ll))
        assert np.all(np.isnan(out[:, 2, 1:L:2]))
    dx, dy = R.detections(zx, zy, K, 5)
    for S, noise in ((AI, float(np.float32(q))), (AA, R.aniso_covs(q, 77)["kappa(Q)=10000"]), (AD, R.detection_covs(K, 6, q))):
        assoc, st = S.associate(rows, *pose, None, dx, dy, noise, GATE, NEW_GATE, 1, L=L, assoc_stride=R.padded(L))
        assert st[:, 0].sum() > 0 and (assoc[:, 1:L:2] != AI.NONE).any()
        out, ll = S.update(rows, *pose, None, assoc, dx, dy, noise, L=L)
        assert np.all(np.isfinite(out[:, :2, :L])) and np.all(np.isfinite(ll))
