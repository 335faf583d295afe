"""The 2x2 noise-form kernels on the regime populations of tests/_regimes.py (test_regimes_spec_cpu.py proves on the CPU that the
populations are what they claim and that the specifications alone keep their float64 bounds on them): every engine-level entry
point of the general-covariance update, the three associations and their updates, the merge and the known-map localisation
against its specification BIT FOR BIT where ekf_rcp takes its division branch in every lane (`high`, `low`), in some lanes of a
wavefront (`mixed`) and in none (`ordinary`), with |pose| up to 1e3 and headings at +-2e4; the DEVICE's results through the same
float64 bound functions; every stored posterior positive definite; unobserved and padding columns untouched in place; every
output bit-identical on a second run.  In front of every launch the population's claim is asserted on the very input
(_regimes.census).  Those populations cannot tell WHICH branch ran (both give the correctly rounded reciprocal there); the last
test does, on determinants of 2^126 and beyond.  The worst error / bound ratios are printed per stage (DESIGN.md section 7 records them)."""
import numpy as np
import pytest
import torch

import _aniso_spec as A
import _assoc_aniso_spec as AA
import _assoc_detcov_spec as AD
import _assoc_spec as AI
import _localise_detcov_spec as LD
import _localise_miss_spec as LM
import _localise_spec as LS
import _merge_spec as M
import _regimes as R
import oracle
from __graft_entry__ import load_package
from _aniso_bounds import check, cov_domain
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
GATE, NEW_GATE, MERGE_GATE, CMAX = 9.21, 50.0, 9.0, 200
SHAPES, CASES, IDS, q_of, seed_of = R.SHAPES, R.CASES, R.CASE_IDS, R.q_of, R.seed_of   # (shared with test_regimes_spec_cpu.py)


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


def same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def twice(run):
    """Every output of a launch is bit-identical on a second run."""
    first, second = run(), run()
    for a, b in zip(first, second):
        assert same(a, b), "a second run gave other bits"
    return first


# ---------------------------------------------------------------- the general-covariance update
@pytest.mark.parametrize("pop,shape", CASES, ids=IDS)
def test_aniso_update(eng, pop, shape):
    n, L, _ = shape
    q, Lp = q_of(pop, shape), R.padded(L)
    worst = {}
    for j in range(2):
        name, cov, pose, rows, zx, zy, det = R.aniso_case(pop, shape, j)
        R.census(pop, det, f"{pop} {name}")
        x, y, th = pose
        anc = np.random.default_rng(n + L).integers(0, n, n).astype(np.int32)
        dx, dy, dth, danc, d_in = dev(x), dev(y), dev(th), dev(anc), dev(rows)
        for pattern in ("all", "third"):
            ids = (np.arange(L) if pattern == "all" else np.arange(0, L, 3)).astype(np.int32)
            eng.obs_upload(ids, zx[ids], zy[ids], L)
            for form in ("gather", "identity", "inplace"):
                label = f"aniso update {pop} n={n} L={L} q={q:g} {name} obs={pattern} {form}"
                a = anc if form == "gather" else None
                want, want_ll = A.update(rows, x, y, th, a, ids, zx[ids], zy[ids], cov, L=L, in_place=form == "inplace")

                def run():
                    d_ll = torch.empty(n, device=DEV)
                    if form == "inplace":
                        d_out = d_in.clone()
                        eng.ekf_update_aniso_dev(d_out, d_out, 5 * Lp, Lp, L, dx, dy, dth, None, n, cov, d_ll)
                    else:
                        d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
                        eng.ekf_update_aniso_dev(d_in, d_out, 5 * Lp, Lp, L, dx, dy, dth, danc if a is not None else None, n, cov, d_ll)
                    return host(d_out), host(d_ll)

                got, got_ll = twice(run)
                assert np.array_equal(bits(got[:, :, :L]), bits(want[:, :, :L])), f"{label}: rows"
                assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: log-likelihoods"
                assert np.all(np.isfinite(got[:, :, ids])) and R.positive_definite(got, ids).all(), f"{label}: a posterior is not positive definite"
                if form == "inplace":
                    rest = np.setdiff1d(np.arange(Lp), ids)
                    assert np.array_equal(bits(got[:, :, rest]), bits(rows[:, :, rest])), f"{label}: unobserved or padding columns changed"
                if pattern == "all" and form == "identity":   # the device's own results against float64
                    body = rows[:, :, :L]
                    w = check(body, got[:, :, :L], got_ll, pose, zx, zy, cov, label, normal=j == 0,
                              domain=cov_domain(body[:, 2], body[:, 3], body[:, 4], cov))
                    worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
        assert np.array_equal(bits(host(d_in)), bits(rows)), "the source rows of an out-of-place update changed"
    print(f"REGIMES aniso update {pop} n={n} L={L} q={q:g}: worst device error / bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------- association and its update, the three noise forms
SPEC = {"iso": AI, "aniso": AA, "detcov": AD}


@pytest.mark.parametrize("form", ("iso", "aniso", "detcov"))
@pytest.mark.parametrize("pop,shape", CASES, ids=IDS)
def test_association_and_its_update(eng, pop, shape, form):
    n, L, K = shape
    q, Lp = q_of(pop, shape), R.padded(L)
    pose, rows, zx, zy, noise, per_k, det = R.assoc_case(pop, shape, form)
    R.census(pop, det, f"{pop} {form}")
    x, y, th = pose
    S = SPEC[form]
    anc = np.random.default_rng(n + L + K).integers(0, n, n).astype(np.int32)
    d_pose, d_rows, d_anc = (dev(x), dev(y), dev(th)), dev(rows), dev(anc)
    eng.detections_upload(zx, zy)
    if form == "detcov":
        eng.detections_cov_upload(*noise)
    head = () if form == "detcov" else (noise,)
    associate = {"iso": eng.associate_dev, "aniso": eng.associate_aniso_dev, "detcov": eng.associate_detcov_dev}[form]
    update = {"iso": eng.ekf_update_assoc_dev, "aniso": eng.ekf_update_assoc_aniso_dev, "detcov": eng.ekf_update_assoc_detcov_dev}[form]
    worst, total = {}, np.zeros(3, np.int64)
    for a in (None, anc):
        label = f"{form} association {pop} n={n} L={L} K={K} q={q:g} anc={a is not None}"
        want, want_st = S.associate(rows, x, y, th, a, zx, zy, noise, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)

        def run_table():
            d_assoc = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
            d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
            associate(d_rows, 5 * Lp, Lp, L, *d_pose, d_anc if a is not None else None, n, *head, GATE, NEW_GATE, 1, d_assoc, Lp, d_st)
            return host(d_assoc), host(d_st)

        got, got_st = twice(run_table)
        assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
        assert np.array_equal(got_st, want_st), f"{label}: counts"
        total += want_st.sum(axis=0)
        d_assoc = dev(want)
        for in_place in ((False,) if a is not None else (False, True)):
            want_rows, want_ll = S.update(rows, x, y, th, a, want, zx, zy, noise, L=L, in_place=in_place)

            def run_update():
                d_ll = torch.empty(n, device=DEV)
                if in_place:
                    d_out = d_rows.clone()
                    update(d_out, d_out, 5 * Lp, Lp, L, *d_pose, None, n, *head, d_assoc, Lp, d_ll)
                else:
                    d_out = torch.full((n, 5, Lp), 7.0, device=DEV)
                    update(d_rows, d_out, 5 * Lp, Lp, L, *d_pose, d_anc if a is not None else None, n, *head, d_assoc, Lp, d_ll)
                return host(d_out), host(d_ll)

            out, ll = twice(run_update)
            assert np.array_equal(bits(out[:, :, :L]), bits(want_rows[:, :, :L])), f"{label} in_place={in_place}: rows"
            assert np.array_equal(bits(ll), bits(want_ll)), f"{label} in_place={in_place}: log-likelihoods"
            if in_place:
                keep = np.ones((n, Lp), bool)
                keep[:, :L] = want[:, :L] == AI.NONE
                keep = np.broadcast_to(keep[:, None, :], out.shape)
                assert np.array_equal(bits(out[keep]), bits(rows[keep])), f"{label}: columns without an association changed"
            src = rows if a is None else rows[a]
            w = R.pairs_check(src, out, ll, pose, want, zx, zy, per_k, L, f"{label} in_place={in_place} (device)")
            worst = {k: max(v, worst.get(k, 0.0)) for k, v in w.items()}
    assert np.array_equal(bits(host(d_rows)), bits(rows)), "the source rows changed"
    assert total[0] + total[1] > 0 or K * n < 4
    print(f"REGIMES {form} association {pop} n={n} L={L} K={K} q={q:g}: matched {total[0]} created {total[1]} dropped {total[2]}; "
          "worst device error / bound " + "  ".join(f"{k} {v:.3g}" for k, v in worst.items()))


# ---------------------------------------------------------------- the merge
@pytest.mark.parametrize("pop,shape", CASES, ids=IDS)
def test_merge(eng, pop, shape):
    n, L, K = shape
    q, Lp = q_of(pop, shape), R.padded(L)
    mp, tab, ev = R.merge_case_of(pop, shape)
    R.merge_census(pop, mp, tab, K, L, f"{pop} merge")
    want_mp, want_ev, want_st = M.merge(mp, tab, K, MERGE_GATE, ev, CMAX, L=L)
    eng.detections_upload(np.zeros(K, F), np.zeros(K, F))

    def run():
        d_mp, d_ev = dev(mp), dev(ev)
        d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
        eng.landmark_merge_dev(d_mp, 5 * Lp, Lp, L, n, dev(tab), L, d_ev, L, CMAX, MERGE_GATE, d_st)
        return host(d_mp), host(d_ev), host(d_st)

    got_mp, got_ev, got_st = twice(run)
    label = f"merge {pop} n={n} L={L} K={K} q={q:g}"
    assert np.array_equal(got_st, want_st), f"{label}: merged / refused / seen differ at {np.argwhere(got_st != want_st)[:5].tolist()}"
    assert np.array_equal(bits(got_mp), bits(want_mp)), f"{label}: rows differ at {np.argwhere(bits(got_mp) != bits(want_mp))[:5].tolist()}"
    assert np.array_equal(got_ev, want_ev), f"{label}: evidence"
    w = R.merge_check(mp, got_mp, tab, K, L, f"{label} (device)")
    print(f"REGIMES {label}: merged {want_st[:, 0].sum()} refused {want_st[:, 1].sum()}; {w['checked']} pairs against float64, "
          f"worst device error / bound mean {w['mean']:.3g}  cov {w['cov']:.3g}")
    if n >= 65:
        assert w["checked"] > 0, f"{label}: no fused pair inside the bound's domain"
    if n * min(K, L // 2) >= 16:
        assert want_st[:, 0].sum() > 0


# ---------------------------------------------------------------- the known map: prepare and localise
def raw_map(Mk, Lp):
    raw = np.zeros((5, Lp), np.float32)
    raw[2] = -1.0
    raw[:, :Mk.shape[1]] = Mk
    return raw


@pytest.mark.parametrize("form", ("iso", "detcov"))
@pytest.mark.parametrize("pop,shape", CASES, ids=IDS)
def test_known_map_prepare_and_localise(eng, pop, shape, form):
    n, L, K = shape
    q, Lp = q_of(pop, shape), (L + 31) // 32 * 32
    pkg = load_package()
    iso = form == "iso"
    Mk, x, y, th, zx, zy, noise, per_k, det = R.localise_case(pop, shape, form)
    R.census(pop, det, f"{pop} localise {form}")
    label = f"localise {form} {pop} n={n} L={L} K={K} q={q:g}"
    d_raw, d_pose = dev(raw_map(Mk, Lp)), (dev(x), dev(y), dev(th))
    eng.detections_upload(zx, zy)
    if iso:
        def run_prepare():
            d_prep = torch.full((6, Lp), 3.0, dtype=torch.float32, device=DEV)
            eng.known_map_prepare_dev(d_raw, Lp, L, noise, d_prep)
            return (host(d_prep),)

        (prep,) = twice(run_prepare)
        with np.errstate(all="ignore"):
            seen, mx, my, i00, i01, i11 = (a[0] for a in AI.shared(Mk[None], noise))
            det = R.dets_iso(Mk[None], noise)[0]
            hl = F(0.5) * oracle.det_log(np.ascontiguousarray(det[seen]))
        for p, want in enumerate((mx, my, i00, i01, i11)):
            assert np.array_equal(bits(prep[p, :L][seen]), bits(want[seen])), f"{label}: prepared plane {p}"
        assert np.array_equal(bits(prep[5, :L][seen]), bits(hl)), f"{label}: prepared 0.5 log det S"
        assert np.all(np.isfinite(prep[2:, :L][:, seen])) and np.all(np.isnan(prep[0, :L][~seen])) and np.all(np.isnan(prep[0, L:]))
        d_map = dev(prep)
    else:
        eng.detections_cov_upload(*noise)
        d_map = d_raw
    want, want_st, want_ll = (LS if iso else LD).localise(Mk, x, y, th, zx, zy, noise, GATE, 0.0)

    def run(table=True):
        d_assoc = torch.full((n, L), 7, dtype=torch.uint8, device=DEV) if table else None
        d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
        d_ll = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
        (eng.localise_dev if iso else eng.localise_detcov_dev)(d_map, Lp, L, *d_pose, n, GATE, d_assoc, L, d_st, d_ll)
        return (host(d_assoc) if table else np.zeros(0, np.uint8)), host(d_st), host(d_ll)

    got, got_st, got_ll = twice(run)
    assert np.array_equal(got, want), f"{label}: table differs at {np.argwhere(got != want)[:5].tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(bits(got_ll), bits(want_ll)), f"{label}: ll differs at {np.flatnonzero(bits(got_ll) != bits(want_ll))[:5].tolist()}"
    _, st2, ll2 = run(table=False)
    assert np.array_equal(st2, want_st) and np.array_equal(bits(ll2), bits(want_ll)), f"{label}: without a table pointer"
    ratio = R.localise_check(Mk, got_ll, (x, y, th), got, zx, zy, per_k, f"{label} (device)")

    # the miss counting (range only: no arc, no line of sight): the same table, stats and ll, and the spec's counts
    view_range = 1e3
    w = LM.localise(Mk, x, y, th, zx, zy, noise, GATE, 0.0, 0.0, (view_range, None, None), None)

    def run_miss():
        d_assoc = torch.full((n, L), 7, dtype=torch.uint8, device=DEV)
        d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
        d_ll = torch.full((n,), 5.0, dtype=torch.float32, device=DEV)
        d_cnt = [torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(3)]
        view = pkg.LocaliseView(view_range, float(LM.ALL[0]), float(LM.ALL[1]), 0, 0.0)
        (eng.localise_miss_dev if iso else eng.localise_detcov_miss_dev)(d_map, Lp, L, *d_pose, n, GATE, d_assoc, L, d_st, d_ll, view, *d_cnt)
        return (host(d_assoc), host(d_st), host(d_ll)) + tuple(host(c) for c in d_cnt)

    g = twice(run_miss)
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1]) and np.array_equal(bits(g[2]), bits(w[2])), f"{label}: the miss form"
    for j, name in ((3, "missed"), (4, "spared"), (5, "outside")):
        assert np.array_equal(g[j], w[j]), f"{label}: {name}"
    print(f"REGIMES {label}: matched {want_st[:, 0].sum()} of {n * K}; worst device |ll - ll_64| / bound {ratio:.3g}")


# ---------------------------------------------------------------- where the reciprocal's two branches differ
def same_or_nan(got, want):
    return (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))


@pytest.mark.parametrize("shape", ((3, 129, 17), (65, 257, 64)), ids=lambda s: f"n{s[0]}-L{s[1]}-K{s[2]}")
def test_determinants_only_the_division_gets_right(eng, shape):
    """The `edge` population (tests/_regimes.py): det S in [2^126, 2^128), whose reciprocal is a denormal number, and det S = +inf,
    whose reciprocal is 0 — bit for bit against the specifications, no float64 bound.  Inside [2^-126, 2^126] the fast chain IS the
    correctly rounded reciprocal, so `high` and `low` cannot tell which branch ran; here they part: with det S = +inf division
    gives 1 / det = 0, S^-1 = 0, the mean w, a Mahalanobis term 0 (a candidate for every detection) and a finite
    log-likelihood, where the fast chain gives NaN throughout.  The posterior covariance of such a lane is 0 * inf = NaN under
    both specifications and kernels (NaN compares as NaN, whatever its payload); every other value is compared by its bits."""
    n, L, K = shape
    pop, q, Lp = "edge", 1e-2, R.padded(L)
    covs2 = R.aniso_covs(q, 77)
    pose, rows, zx, zy = R.frame(pop, n, L, q, 4242 + L, Lp=Lp)
    x, y, th = pose
    d_pose, d_rows = (dev(x), dev(y), dev(th)), dev(rows)
    overflow = np.isinf(R.dets_iso(rows[:, :, :L], q))
    assert overflow[:, 1::2].all() and not overflow[:, 0::2].any()
    # the general-covariance update
    ids = np.arange(L, dtype=np.int32)
    eng.obs_upload(ids, zx, zy, L)
    for name, cov in covs2.items():
        R.census(pop, R.dets_aniso(rows[:, :, :L], th, cov), f"edge {name}")
        want, want_ll = A.update(rows, x, y, th, None, ids, zx, zy, cov, L=L)
        assert np.all(np.isfinite(want[:, :, 0:L:2])) and np.all(np.isfinite(want[:, :2, :L])) and np.all(np.isfinite(want_ll))
        assert np.all(np.isnan(want[:, 2, 1:L:2]))
        for in_place in (False, True):
            def run():
                d_ll = torch.empty(n, device=DEV)
                d_out = d_rows.clone() if in_place else torch.full((n, 5, Lp), 7.0, device=DEV)
                eng.ekf_update_aniso_dev(d_out if in_place else d_rows, d_out, 5 * Lp, Lp, L, *d_pose, None, n, cov, d_ll)
                return host(d_out), host(d_ll)
            got, got_ll = twice(run)
            assert same_or_nan(got[:, :, :L], want[:, :, :L]).all(), f"edge aniso update {name} in_place={in_place}: rows"
            assert np.array_equal(bits(got_ll), bits(want_ll)), f"edge aniso update {name} in_place={in_place}: log-likelihoods"
    # the three associations and their updates
    dx, dy = R.detections(zx, zy, K, 5)
    eng.detections_upload(dx, dy)
    dcov = R.detection_covs(K, 6, q)
    eng.detections_cov_upload(*dcov)
    for form, noise in (("iso", float(F(q))), ("aniso", covs2["kappa(Q)=10000"]), ("detcov", dcov)):
        S = SPEC[form]
        head = () if form == "detcov" else (noise,)
        associate = {"iso": eng.associate_dev, "aniso": eng.associate_aniso_dev, "detcov": eng.associate_detcov_dev}[form]
        update = {"iso": eng.ekf_update_assoc_dev, "aniso": eng.ekf_update_assoc_aniso_dev, "detcov": eng.ekf_update_assoc_detcov_dev}[form]
        want, want_st = S.associate(rows, x, y, th, None, dx, dy, noise, GATE, NEW_GATE, 1, L=L, assoc_stride=Lp)
        assert want_st[:, 0].sum() > 0 and (want[:, 1:L:2] != AI.NONE).any()      # landmarks with det S = inf take detections

        def run_table():
            d_assoc = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
            d_st = torch.full((n, 3), -1, dtype=torch.int32, device=DEV)
            associate(d_rows, 5 * Lp, Lp, L, *d_pose, None, n, *head, GATE, NEW_GATE, 1, d_assoc, Lp, d_st)
            return host(d_assoc), host(d_st)

        got, got_st = twice(run_table)
        assert np.array_equal(got, want), f"edge {form}: table differs at {np.argwhere(got != want)[:5].tolist()}"
        assert np.array_equal(got_st, want_st), f"edge {form}: counts"
        want_rows, want_ll = S.update(rows, x, y, th, None, want, dx, dy, noise, L=L)
        assert np.all(np.isfinite(want_rows[:, :2, :L])) and np.all(np.isfinite(want_ll))

        def run_update():
            d_ll, d_out = torch.empty(n, device=DEV), torch.full((n, 5, Lp), 7.0, device=DEV)
            update(d_rows, d_out, 5 * Lp, Lp, L, *d_pose, None, n, *head, dev(want), Lp, d_ll)
            return host(d_out), host(d_ll)

        out, ll = twice(run_update)
        assert same_or_nan(out[:, :, :L], want_rows[:, :, :L]).all(), f"edge {form}: rows"
        assert np.array_equal(bits(ll), bits(want_ll)), f"edge {form}: log-likelihoods"
