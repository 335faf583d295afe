"""Regime populations for the kernels that do their 2x2 arithmetic with ekf_rcp / det_logf / det_sincosf (csrc/ekf_math.h): the
general-covariance update, the three associations and their updates, the merge and the known-map localisation.  TEST
INFRASTRUCTURE shared by test_regimes_spec_cpu.py (the specifications alone, no GPU) and test_gpu_regimes.py (the kernels); built
on _f64_pf.GRID / random_priors / regime_frame / mixed_frame — no other grid.

ekf_rcp takes the fast reciprocal only if EVERY lane of the wavefront holds a determinant with 2^-60 <= |det| < 2^61 (a test of
the exponent: NaN and infinity are outside); one lane outside sends the whole wavefront through IEEE division.  Three
populations per (n, L, q):

  ordinary   the grid's (P / q, kappa(P)) regimes at this q, by landmark, restricted to those whose det (P + R) stays inside the
             range under the noise at hand (with kappa(Q) = 1e4 at q = 1e-8 the smallest priors fall below 2^-60 and are left
             out): the fast reciprocal alone.  First sightings P_xx = -1.
  high       every prior ~1e10 m^2 (det ~1e19 >= 2^61): the division branch in every lane of every wavefront.
  low        q = Q_LOW = 2^-32 — the largest power of two for which det (P + q I) <= 4 q^2 < 2^-60 for every P <= q; every entry
             point accepts it — and the grid's regimes with P / q <= 1: det < 2^-60 everywhere.
             In `high` and `low` a first sighting is marked by P_xx = -(the population's scale), not -1: the arithmetic runs on the
             marked lanes too (and is selected away), and -1 would put their determinant back into the range.
  edge       (bit for bit only, no float64 bound) priors of ~1.5e19 m^2, kappa 1.5, so that 2^126 <= det S < 2^128 and 1 / det S
             is a DENORMAL number, alternating by landmark with priors of 3e19 m^2, kappa 1, whose det S overflows to +inf
             (1 / det S = 0).  These are the determinants at which ekf_rcp's two branches stop being interchangeable: inside
             [2^-126, 2^126] the fast chain (estimate + six fused multiply-adds, each rounded once, nothing underflowing) is the
             correctly rounded reciprocal, i.e. the division's bits, so a kernel that took it unconditionally would pass `high`
             and `low`; at +inf it yields fma(-inf, 0, 1) = NaN where division yields 0, and in the denormal range neither the
             estimate nor the last step is guaranteed.  No first sightings.
  mixed      _f64_pf.mixed_frame: the regime changes from landmark to landmark, every 16th landmark carries a ~1e10 m^2 prior on
             half of the even particles (and on particle 0 always), first sightings P_xx = -1.

WHICH AXIS MIXES.  ekf_row_body.h (the row walk of every update form here), match_body.h (associate_body, localise_particle) and
merge_kernels.hip all give ONE PARTICLE TO ONE WAVEFRONT and lay landmarks l, l + 64 of each batch of 128 across the lanes, two
per lane on the packed v2f path: for them the LANDMARK axis produces the mix (landmark 15 of every 16 beside ordinary ones in one
64-lane block; lanes whose pair (l, l + 64) is half in, half out for the packed test).  The merge's lanes hold the FREE landmarks
while a wave-uniform loop walks the anchors: the mix comes from huge free landmarks beside ordinary ones under an ordinary
anchor.  known_map_prepare_kernel lays landmarks across lanes: the landmark axis again.  The grouped kernels (ekf_group_body.h)
lay PARTICLES of one ancestor across lanes: there the mix comes from the particle axis, the huge priors on every other particle;
the engine-level entry points used here take the row walk, the session tests reach the grouped one.
Padding columns [L, Lp) hold junk and NaN as test_gpu_aniso.make_case's: a wavefront that walks them unpredicated takes the
division branch whatever the population — the claim of `ordinary` is about the columns below L.
"""
import numpy as np

import _aniso_spec as AS
import _f64_pf as F
import oracle
from _aniso_bounds import bounds, cov_domain, q_matrix, world_noise64
from _detections import covariances, detections   # noqa: F401 - detections: for the tests

F32 = np.float32
U, SC = F.U, F.SINCOS_ABS
RCP_LO, RCP_HI = 2.0 ** -60, 2.0 ** 61
Q_LOW = 2.0 ** -32
HUGE = 1e10
POPULATIONS = ("ordinary", "high", "low", "mixed")     # (and "edge", compared bit for bit only)
QS = tuple(sorted({q for q, _, _ in F.GRID}))
WAVE = 64


def in_range(det):
    """ekf_rcp_in_range on float32 values: 2^-60 <= |d| < 2^61 by the exponent field."""
    e = ((np.ascontiguousarray(det, np.float32).view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    return (e >= 67) & (e <= 187)


def det_s(pxx, pxy, pyy, rxx, rxy, ryy):
    """det (P + R) as every specification forms it: three sums, two products, one difference, each rounded to float32."""
    with np.errstate(all="ignore"):
        a = (pxx + rxx).astype(F32)
        b = (pxy + rxy).astype(F32)
        cc = (pyy + ryy).astype(F32)
        t = a * cc
        u = b * b
        return (t - u).astype(F32)


def regimes_at(pop, q, q_lo=None):
    """The (P / q, kappa(P)) pairs a population draws its priors from; q_lo: the noise's smallest eigenvalue (default q)."""
    grid = sorted({(r, k) for _, r, k in F.GRID})
    if pop == "high":
        return [(HUGE / q, 10.0)]
    if pop == "edge":
        return [(1.5e19 / q, 1.5), (3e19 / q, 1.0)]
    if pop == "low":
        assert q == Q_LOW
        return [(r, k) for r, k in grid if r <= 1.0]
    q_lo = q if q_lo is None else q_lo
    # lambda_min(S) >= lambda_min(P) + lambda_min(Q), lambda_max(S) >= max(lambda_max(P), lambda_max(Q)); a factor 4 to spare
    return [(r, k) for r, k in grid if (r * q / k + q_lo) * max(r * q, q) >= 4 * RCP_LO and (r * q + q) ** 2 <= RCP_HI / 4]


def poses(rng, n):
    """|x|, |y|, |theta| up to 1e3; a handful of headings at +-2e4, the edge of det_sincosf's stated domain."""
    x, y, th = (rng.uniform(-1e3, 1e3, n).astype(F32) for _ in range(3))
    edge = np.arange(n)[2::13]
    th[edge] = np.where(np.arange(len(edge)) % 2 == 0, 2e4, -2e4).astype(F32)
    return x, y, th


def frame(pop, n, L, q, seed, Lp=None, q_lo=None, pose=None):
    """-> (pose (x, y, theta), rows float32 [n][5][Lp], zx, zy [L]): one observation per landmark, every particle's prior mean
    a draw from its own covariance around the point it observes (q = Q_LOW for `low`)."""
    rng = np.random.default_rng(seed)
    Lp = L if Lp is None else Lp
    pose = poses(rng, n) if pose is None else pose
    if pop == "mixed":
        pose, body, zx, zy = F.mixed_frame(rng, n, L, q, pose=pose)
        if L > 15:                                                   # particle 0, landmark 15: always a huge prior beside ordinary ones
            body[0, 2, 15], body[0, 3, 15], body[0, 4, 15] = (v[0] for v in F.random_priors(rng, (1,), 1.0, HUGE, 10.0))
    else:
        regs = regimes_at(pop, q, q_lo)
        body, zx, zy = np.empty((n, 5, L), F32), np.empty(L, F32), np.empty(L, F32)
        for j, (r, k) in enumerate(regs):
            cols = np.arange(j, L, len(regs))
            if len(cols):
                pose, body[:, :, cols], zx[cols], zy[cols] = F.regime_frame(rng, n, len(cols), q, r, k, pose=pose)
        if pop != "edge":
            mark = {"ordinary": -1.0, "high": -HUGE, "low": -Q_LOW * 2.0 ** -14}[pop]
            body[:, 2][rng.random((n, L)) < 0.1] = mark
    rows = np.empty((n, 5, Lp), F32)
    rows[:, :, :L] = body
    pad = rng.standard_normal((n, 5, Lp - L)).astype(F32) * 1e3
    pad[rng.random(pad.shape) < 0.2] = np.nan
    rows[:, :, L:] = pad
    return pose, rows, zx, zy


def aniso_covs(q, seed):
    """The anisotropic form's Q at this q: kappa(Q) in {1, 1e4}, lambda_max(Q) = q, the axes turned."""
    rng = np.random.default_rng(seed)
    return {f"kappa(Q)={k:g}": q_matrix(q, k, rng.uniform(0, np.pi)) for k in (1.0, 1e4)}


def detection_covs(K, seed, q):
    """_detections.covariances (the construction of test_gpu_assoc_detcov.py) scaled to q: every Q_k different, lambda_max within
    a decade below q, a : b up to 1 : 1e4."""
    return covariances(K, seed, qm=q)


DETCOV_Q_LO = 1e-5    # ... so lambda_min(Q_k) >= q * 1e-1 * 1e-4


def sincos(th):
    return oracle.det_sincos(np.ascontiguousarray(th, F32))


def dets_iso(body, q):
    z = F32(0.0)
    return det_s(body[:, 2], body[:, 3], body[:, 4], F32(q), z, F32(q))


def dets_aniso(body, th, cov):
    """[n][L]: det (P + R_w(theta_i)) of every (particle, landmark)."""
    s, c = sincos(th)
    rxx, rxy, ryy = AS.world_noise(cov, s, c)
    return det_s(body[:, 2], body[:, 3], body[:, 4], rxx[:, None], rxy[:, None], ryy[:, None])


def dets_detcov(body, th, covs):
    """[n][L][K]: det (P + R_w(theta_i, k)) of every (particle, landmark, detection)."""
    s, c = sincos(th)
    out = np.empty(body.shape[:1] + body.shape[2:] + (len(covs[0]),), F32)
    for k in range(len(covs[0])):
        rxx, rxy, ryy = AS.world_noise((covs[0][k], covs[1][k], covs[2][k]), s, c)
        out[:, :, k] = det_s(body[:, 2], body[:, 3], body[:, 4], rxx[:, None], rxy[:, None], ryy[:, None])
    return out


def census(pop, det, label=""):
    """The population is what it claims: det [n][L(, ...)] float32 as the specification computes it.  ordinary: none outside the
    range; high / low: all outside; mixed: some 64-landmark block of some particle holds both kinds.  -> the share outside."""
    ok = in_range(det)
    ok = ok.reshape(ok.shape[0], ok.shape[1], -1)
    out = (~ok).mean()
    if pop == "ordinary":
        assert ok.all(), f"{label}: {int((~ok).sum())} determinants outside the fast reciprocal's range"
    elif pop in ("high", "low", "edge"):
        assert not ok.any(), f"{label}: {int(ok.sum())} determinants inside the fast reciprocal's range"
    else:
        both = False
        for b in range(0, ok.shape[1], WAVE):
            blk = ok[:, b:b + WAVE]
            both |= bool((blk.any(axis=1) & (~blk).any(axis=1)).any())
        assert both, f"{label}: no 64-landmark block with lanes inside and outside the range"
    return float(out)


def positive_definite(out, cols=None):
    """Stored covariances of the seen landmarks: positive definite in float64, from the float32 values."""
    p = np.asarray(out, np.float64)
    p = p if cols is None else p[:, :, cols]
    seen = ~(p[:, 2] < 0)
    return ((p[:, 2] > 0) & (p[:, 4] > 0) & (p[:, 2] * p[:, 4] - p[:, 3] * p[:, 3] > 0)) | ~seen


def pairs_check(src, out, ll, pose, assoc, dx, dy, noise, L, label):
    """An associating update against float64, pair by pair: src / out [n][5][>= L] the rows each particle started from and what
    the update left, assoc [n][>= L] the table (entry < K: the detection landmark l took), noise: a meas_var (the isotropic
    bounds of _f64_pf.update_errors) or K triples Q_k (_aniso_bounds.bounds, each pair with its own quantities).  Created
    landmarks: the observed point within the first-sighting bound; P = q I exactly, or within e_R of R_w.  Every stored posterior
    positive definite.  Prints and returns the worst error / bound ratios."""
    x, y, th = (np.asarray(a) for a in pose)
    n, K = len(x), len(dx)
    iso = np.isscalar(noise)
    worst = dict(mean=0.0, cov=0.0, first=0.0)
    ll64, b_sum, npd = np.zeros(n), np.zeros(n), 0
    for k in range(K):
        ii, lc = np.nonzero(assoc[:, :L] == k)
        if len(ii) == 0:
            continue
        p = src[ii, :, lc].T.astype(np.float64)
        g = out[ii, :, lc].T.astype(np.float64)
        first = p[2] < 0
        seen = ~first
        pp = np.where(seen, p, np.array([0, 0, 1, 0, 1], np.float64)[:, None])
        ps = (x[ii], y[ii], th[ii])
        if iso:
            r = F.update_errors(g, pp, ps, dx[k], dy[k], noise)
            r_mean, r_cov, ref_ll, b_ll = r["mean"], r["cov"], r["ll_ref"], r["b_ll"]
            rw = (float(F32(noise)), 0.0, float(F32(noise)))
            e_r = 0.0
        else:
            cov = tuple(noise[k])
            ref, b = bounds(pp, ps, dx[k], dy[k], cov)
            r_mean = np.hypot(g[0] - ref[0], g[1] - ref[1]) / b["mean"]
            r_cov = np.maximum(np.maximum(np.abs(g[2] - ref[2]), np.abs(g[3] - ref[3])), np.abs(g[4] - ref[4])) / b["cov"]
            r_cov = np.where(cov_domain(pp[2], pp[3], pp[4], cov), r_cov, 0.0)      # (beyond it the float64 reference itself is lost)
            ref_ll, b_ll = ref[5], b["ll"]
            rw, e_r = world_noise64(cov, th[ii]), b["e_r"]
        worst["mean"] = max(worst["mean"], float(np.where(seen, r_mean, 0.0).max()))
        worst["cov"] = max(worst["cov"], float(np.where(seen, r_cov, 0.0).max()))
        npd += int((~((g[2] > 0) & (g[4] > 0) & (g[2] * g[4] - g[3] * g[3] > 0))).sum())
        fx, fy = F.first_sighting(dx[k], dy[k], *ps)
        b_first = 4 * U * (np.hypot(ps[0], ps[1]) + np.hypot(fx, fy)) + 4 * (SC + U) * np.hypot(dx[k], dy[k])
        e_first = np.maximum(np.maximum(np.abs(g[2] - rw[0]), np.abs(g[3] - rw[1])), np.abs(g[4] - rw[2]))
        r_first = np.hypot(g[0] - fx, g[1] - fy) / b_first
        if iso:
            assert np.all(e_first[first] == 0), f"{label}: a created landmark's P is not q I"
        else:
            r_first = np.maximum(r_first, e_first / e_r)
        worst["first"] = max(worst["first"], float(np.where(first, r_first, 0.0).max()))
        t = np.where(seen, ref_ll, 0.0)
        ll64 += np.bincount(ii, t, minlength=n)
        b_sum += np.bincount(ii, np.where(seen, b_ll, 0.0) + (-(-L // 128) + 7) * U * np.abs(t), minlength=n)
    worst["loglik"] = float((np.abs(np.asarray(ll, np.float64) - ll64) / (b_sum + 1e-30)).max())
    print(f"{label}: max error / bound  mean {worst['mean']:.3g}  cov {worst['cov']:.3g}  first {worst['first']:.3g}  "
          f"loglik {worst['loglik']:.3g}; non-positive-definite posteriors {npd}")
    for name, v in worst.items():
        assert v <= 1.0, f"{label}: {name} error {v:.3g} x its bound"
    assert npd == 0, f"{label}: {npd} posteriors not positive definite"
    return worst


# ---------------------------------------------------------------- the merge
def merge_case(pop, n, L, Lp, K, q, seed):
    """Rows as an associating update leaves them, for slam_landmark_merge_dev: anchor j of a particle in slot 2 j (named by the
    table), its duplicate — a free landmark within the gate, d a draw from 0.49 S — in slot 2 j + 1; the slots behind them are
    further free duplicates of anchors in turn, every seventh a covariance that is not positive definite ON its anchor (the
    guard's refusal) and, in `ordinary` and `mixed`, every fifth unseen.  P_l and P_w come from the population's regimes at scale
    q (`high`: ~1e10 m^2; `low`: q = Q_LOW, P <= q, so det (P_l + P_w) <= 4 q^2 < 2^-60; `mixed`: every 16th FREE landmark of the
    even particles huge — and free landmark 15 of particle 0 always — beside ordinary ones under ordinary anchors).
    -> (mp [n][5][Lp], tab uint8 [n][L], ev uint8 [n][L])."""
    rng = np.random.default_rng(seed)
    base = "ordinary" if pop == "mixed" else pop
    regs = regimes_at(base, q)
    if base == "ordinary":      # no noise holds S up here: det S >= det P_l + det P_w, each (r q)^2 / k, and S <= 2 max(P_l, P_w)
        regs = [(r, k) for r, k in regs if (r * q) ** 2 / k >= 4 * RCP_LO and (2 * r * q) ** 2 <= RCP_HI / 4]
    na = min(K, L // 2)
    mp = (rng.standard_normal((n, 5, Lp)) * 1e3).astype(F32)
    mp[rng.random(mp.shape) < 0.2] = np.nan
    tab = np.full((n, L), 255, np.uint8)
    ev = rng.integers(0, 256, (n, L)).astype(np.uint8)
    if na == 0:
        mp[:, 2, :L] = -1.0
        return mp, tab, ev

    def draw(shape, j):
        r, k = regs[j % len(regs)]
        return np.stack(F.random_priors(rng, shape, q, r, k)).astype(np.float64)

    slots = np.arange(L)
    anchor_of = np.where(slots < 2 * na, slots // 2, (slots * 7 + 3) % na)
    is_anchor = (slots < 2 * na) & (slots % 2 == 0)
    pw = np.stack([draw((n,), j) for j in range(na)], axis=-1)                 # [3][n][na]
    mw = rng.uniform(-1e3, 1e3, (2, n, na))
    order = rng.permutation(K)[:na]
    for l in slots:
        j = int(anchor_of[l])
        if is_anchor[l]:
            mp[:, 0, l], mp[:, 1, l] = mw[0, :, j], mw[1, :, j]
            mp[:, 2, l], mp[:, 3, l], mp[:, 4, l] = pw[0, :, j], pw[1, :, j], pw[2, :, j]
            tab[:, l] = order[j]
            continue
        pl = draw((n,), l + 3)
        if pop == "mixed" and l % 16 == 15:
            huge = np.stack(F.random_priors(rng, (n,), 1.0, HUGE, 10.0)).astype(np.float64)
            sel = (np.arange(n) % 2 == 0) & (rng.random(n) < 0.5)
            sel[0] = sel[0] or l == 15
            pl = np.where(sel[None], huge, pl)
        s00, s01, s11 = pl[0] + pw[0, :, j], pl[1] + pw[1, :, j], pl[2] + pw[2, :, j]
        l00 = np.sqrt(s00)
        l10 = s01 / l00
        l11 = np.sqrt(np.maximum(s11 - l10 * l10, 0.0))
        g = rng.standard_normal((2, n)) * (0.7 if l < 2 * na else 1.2)
        mp[:, 0, l] = mw[0, :, j] + l00 * g[0]
        mp[:, 1, l] = mw[1, :, j] + l10 * g[0] + l11 * g[1]
        mp[:, 2, l], mp[:, 3, l], mp[:, 4, l] = pl
        if l >= 2 * na and l % 7 == 0:                                            # not positive definite, on its anchor
            sc = np.maximum(pw[0, :, j], pw[2, :, j])
            mp[:, 0, l], mp[:, 1, l] = mw[0, :, j], mw[1, :, j]
            mp[:, 2, l], mp[:, 3, l], mp[:, 4, l] = 0.05 * sc, 0.2 * sc, 0.05 * sc
        elif l >= 2 * na and l % 5 == 0 and l % 16 != 15 and pop in ("ordinary", "mixed"):
            mp[:, 2, l] = -1.0
    return mp, tab, ev


def dets_merge(mp, tab, K, L):
    """[n][L][anchors]: det (P_l + P_w) of every (slot, anchor) pair the stage forms, as _merge_spec.shared_pair rounds it."""
    import _merge_spec as M
    _, anchor, _ = M.roles(mp, tab, K, L)
    na = int(anchor.sum(axis=1).max(initial=0))
    out = np.empty((mp.shape[0], L, na), F32)
    for i in range(mp.shape[0]):
        w = np.flatnonzero(anchor[i])
        out[i] = det_s(mp[i, 2, w][None, :], mp[i, 3, w][None, :], mp[i, 4, w][None, :], mp[i, 2, :L, None], mp[i, 3, :L, None], mp[i, 4, :L, None])
    return out


def merged_pairs(mp, out, tab, K, L):
    """The pairs a merge fused, read off its result: (particle, absorbed slot, anchor) arrays.  The absorbed slot is a seen slot
    that came out cleared; its anchor is the one it chose by the specification's rule (the cheapest, the lowest on ties)."""
    import _merge_spec as M
    _, anchor, _ = M.roles(mp, tab, K, L)
    cleared = (out[:, 2, :L] < 0) & ~(mp[:, 2, :L] < 0)
    ii, ls, ws = [], [], []
    for i, l in zip(*np.nonzero(cleared)):
        w = np.flatnonzero(anchor[i])
        with np.errstate(all="ignore"):
            m = M.pair_cost(tuple(mp[i, p, l] for p in range(5)), tuple(mp[i, p, w] for p in range(5)))
        m = np.where(np.isnan(m), np.inf, m)
        ii.append(i), ls.append(l), ws.append(w[int(np.argmin(m))])
    return np.array(ii, np.int64), np.array(ls, np.int64), np.array(ws, np.int64)


def merge_check(mp, out, tab, K, L, label):
    """The fused anchors of a merge against the float64 information form (_merge_bounds.fusion_check); positive definite."""
    from _merge_bounds import fusion_check
    ii, ls, ws = merged_pairs(mp, out, tab, K, L)
    if len(ii) == 0:
        print(f"{label}: nothing was fused: nothing checked against float64")
        return dict(mean=float("nan"), cov=float("nan"), checked=0)
    o = out[ii, :, ws].T.astype(np.float64)
    ml, pl = mp[ii, :2, ls].T, mp[ii, 2:, ls].T
    mw, pw = mp[ii, :2, ws].T, mp[ii, 2:, ws].T
    assert np.all((o[2] > 0) & (o[4] > 0) & (o[2] * o[4] - o[3] * o[3] > 0)), f"{label}: a fused anchor is not positive definite"
    # THE BOUND'S DOMAIN.  It charges every operation a relative error u, which holds for results in the normal range.  A product
    # that underflows gradually carries an ABSOLUTE error of up to 2^-150 instead.  The fusion's products are those of det P_w and
    # det P_l (two each) and the six det P * P' of the covariance's numerators; each error reaches P' through at most
    # max(1, lambda) / det S, so with no measurement noise to hold the scale up the underflows add at most 8 * 2^-150 / det S to an
    # entry of P' (covariances below 1 m^2).  The bound says nothing about that term; it is kept below one u of the result,
    #     8 * 2^-150 / det S <= u lambda_max(P')   <=>   det S * lambda_max(P') >= 2^-123,
    # which for P_l ~ P_w ~ P reads P^3 >= 2^-124: the pairs of the `low` population with kappa(P) >= 1e2 at P / q = 1e-4 lie
    # beyond it (products really below 2^-126) and are held to bit equality and positive definiteness alone.
    f64 = lambda a: np.asarray(a, np.float64)
    s00, s01, s11 = f64(pl[0]) + f64(pw[0]), f64(pl[1]) + f64(pw[1]), f64(pl[2]) + f64(pw[2])
    _, lmax_post = F._eig2(o[2], o[3], o[4])
    big = np.maximum(np.maximum(f64(pl[0]), f64(pl[2])), np.maximum(f64(pw[0]), f64(pw[2]))) >= 1.0
    dom = ((s00 * s11 - s01 * s01) * lmax_post >= 2.0 ** -123) | big
    print(f"{label}: {int(dom.sum())} of {len(dom)} fused pairs inside the bound's domain (no underflow)")
    if not dom.any():
        print(f"{label}: NO pair inside the bound's domain: nothing checked against float64")
        return dict(mean=float("nan"), cov=float("nan"), checked=0)
    # (min_use: fusion_check leaves out pairs whose ROUNDED inputs are no longer positive definite; its 0.9 is the share among
    # test_merge_spec_cpu.py's random regimes.  Here whole shapes sit at kappa(P) = 1e4, where rounding costs more of them.)
    w = fusion_check(o[:, dom], ml[:, dom], pl[:, dom], mw[:, dom], pw[:, dom], min_use=0.5, label=label)
    return dict(w, checked=int(dom.sum()))


# ---------------------------------------------------------------- the known map
def known_map_case(pop, n, L, K, q, seed, q_lo=None):
    """A known map whose landmarks carry the population's regimes, a true pose up to 1e3 from the origin that sees K of them, and a
    cloud of n particles on and around that pose (particles 0 and 1 exactly on it; a handful of headings at +-2e4).  The map is
    particle 0's row of frame(): means drawn from each landmark's covariance around the point the true pose observes; the slots
    frame() marks as first sightings hold no landmark.  -> (M [5][L], x, y, th [n], zx, zy [K])."""
    rng = np.random.default_rng(seed + 17)
    x0, y0, th0 = (rng.uniform(-1e3, 1e3, 2).astype(F32) for _ in range(3))
    pose, rows, zx, zy = frame(pop, 2, L, q, seed, q_lo=q_lo, pose=(x0, y0, th0))
    M = np.ascontiguousarray(rows[0, :, :L])
    x = (x0[0] + 2e-3 * rng.standard_normal(n)).astype(F32)
    y = (y0[0] + 2e-3 * rng.standard_normal(n)).astype(F32)
    th = (th0[0] + 1e-4 * rng.standard_normal(n)).astype(F32)
    x[:2], y[:2], th[:2] = x0[0], y0[0], th0[0]
    edge = np.arange(n)[5::29]
    th[edge] = np.where(np.arange(len(edge)) % 2 == 0, 2e4, -2e4).astype(F32)
    seen = np.flatnonzero(~(M[2] < 0))
    pick = rng.permutation(seen)[:K]
    dx = np.concatenate([zx[pick], rng.uniform(-1e3, 1e3, K - len(pick)).astype(F32)]).astype(F32)
    dy = np.concatenate([zy[pick], rng.uniform(-1e3, 1e3, K - len(pick)).astype(F32)]).astype(F32)
    return M, x, y, th, dx, dy


def localise_check(M, ll, pose, assoc, dx, dy, noise, label):
    """The log-likelihood of a localise stage against the textbook likelihood of the pairs its table names, in float64: each
    pair's term within its own bound (isotropic: _f64_pf.update_errors' b_ll; per detection: _aniso_bounds.bounds' with Q_k), the
    sum within the sum of those plus the summation tree's (ceil(L / 128) + 7) u sum |ll|.  -> the worst |error| / bound."""
    x, y, th = (np.asarray(a) for a in pose)
    n, L = len(x), M.shape[1]
    iso = np.isscalar(noise)
    ll64, b_sum = np.zeros(n), np.zeros(n)
    for k in range(len(dx)):
        ii, lc = np.nonzero(assoc[:, :L] == k)
        if len(ii) == 0:
            continue
        p = M[:, lc].astype(np.float64)
        ps = (x[ii], y[ii], th[ii])
        if iso:
            r = F.update_errors(p, p, ps, dx[k], dy[k], noise)
            t, b = r["ll_ref"], r["b_ll"]
        else:
            ref, bb = bounds(p, ps, dx[k], dy[k], tuple(noise[k]))
            t, b = ref[5], bb["ll"]
        ll64 += np.bincount(ii, t, minlength=n)
        b_sum += np.bincount(ii, b + (-(-L // 128) + 7) * U * np.abs(t), minlength=n)
    ok = np.isfinite(x) & np.isfinite(th)
    ratio = float(np.max((np.abs(np.asarray(ll, np.float64) - ll64) / (b_sum + 1e-30))[ok], initial=0.0))
    print(f"{label}: max |ll - ll_64| / bound {ratio:.3g} over {int((assoc[:, :L] != 255).sum())} matched pairs")
    assert ratio <= 1.0, f"{label}: log-likelihood {ratio:.3g} x its bound"
    return ratio


# ---------------------------------------------------------------- the cases test_gpu_regimes.py runs (test_regimes_spec_cpu.py
# asserts the populations' claims on exactly these, and the GPU test asserts them again in front of every launch)
# n in {1, 3, 65, 130} x L in {31, 129, 257} x K in {1, 17, 64}: one wavefront and several, a last workgroup that is not full; below,
# across and two past the 128-landmark batch; one detection, an odd count, the most
SHAPES = ((1, 31, 1), (3, 129, 17), (65, 257, 64), (130, 129, 64), (130, 31, 17))
CASES = [(pop, shape) for pop in POPULATIONS for shape in SHAPES]
CASE_IDS = [f"{pop}-n{n}-L{L}-K{K}" for pop, (n, L, K) in CASES]
FORMS = ("iso", "aniso", "detcov")


def q_of(pop, shape):
    """The grid's q in turn over the shapes; `low` has its own."""
    return Q_LOW if pop == "low" else QS[SHAPES.index(shape) % len(QS)]


def seed_of(pop, shape, extra=0):
    return 100 * (POPULATIONS + ("edge",)).index(pop) + 10 * SHAPES.index(shape) + extra + 5000


def padded(L):
    return (L + 32) // 32 * 32


def aniso_case(pop, shape, j):
    """Q number j of aniso_covs -> (name, cov, pose, rows [n][5][Lp], zx, zy, det [n][L])."""
    n, L, _ = shape
    q = q_of(pop, shape)
    name, cov = list(aniso_covs(q, seed_of(pop, shape)).items())[j]
    pose, rows, zx, zy = frame(pop, n, L, q, seed_of(pop, shape, j), Lp=padded(L), q_lo=q / (1.0, 1e4)[j])
    return name, cov, pose, rows, zx, zy, dets_aniso(rows[:, :, :L], pose[2], cov)


def assoc_case(pop, shape, form):
    """-> (pose, rows [n][5][Lp], zx, zy [K], noise as the entry point takes it, K triples or the meas_var, det of every pair)."""
    n, L, K = shape
    q, Lp = q_of(pop, shape), padded(L)
    s = seed_of(pop, shape, 3 + FORMS.index(form))
    if form == "iso":
        pose, rows, zx, zy = frame(pop, n, L, q, s, Lp=Lp)
        noise = per_k = float(F32(q))
        det = dets_iso(rows[:, :, :L], q)
    elif form == "aniso":
        noise = aniso_covs(q, s)["kappa(Q)=10000"]
        per_k = [noise] * K
        pose, rows, zx, zy = frame(pop, n, L, q, s, Lp=Lp, q_lo=q * 1e-4)
        det = dets_aniso(rows[:, :, :L], pose[2], noise)
    else:
        noise = detection_covs(K, s, q)
        per_k = list(zip(*noise))
        pose, rows, zx, zy = frame(pop, n, L, q, s, Lp=Lp, q_lo=q * DETCOV_Q_LO)
        det = dets_detcov(rows[:, :, :L], pose[2], noise)
    return pose, rows, *detections(zx, zy, K, s), noise, per_k, det


def merge_case_of(pop, shape):
    n, L, K = shape
    return merge_case(pop, n, L, padded(L), K, q_of(pop, shape), seed_of(pop, shape, 8))


def merge_census(pop, mp, tab, K, L, label=""):
    """census over the (slot, anchor) pairs of positive definite seen slots: the slots placed to be refused are indefinite, and
    det (P_l + P_w) of an indefinite sum cancels to any magnitude."""
    import _merge_spec as M
    _, anchor, free = M.roles(mp, tab, K, L)
    det = dets_merge(mp, tab, K, L)
    if det.shape[2] == 0:
        return 0.0
    p64 = mp[:, 2:, :L].astype(np.float64)
    part = ((free | anchor) & (p64[:, 0] * p64[:, 2] - p64[:, 1] ** 2 > 0))[:, :, None]
    if pop == "mixed" and L <= 15:
        pop = "ordinary"
    return census(pop, np.where(part, det, F32(1.0 if pop in ("ordinary", "mixed") else 0.0)), label)


def localise_case(pop, shape, form):
    """-> (M [5][L], x, y, th, zx, zy, noise, K triples or the meas_var, det of every pair the stage forms)."""
    n, L, K = shape
    q, s = q_of(pop, shape), seed_of(pop, shape, 9)
    if form == "iso":
        Mk, x, y, th, zx, zy = known_map_case(pop, n, L, K, q, s)
        noise = per_k = float(F32(q))
        det = dets_iso(Mk[None], q)
    else:
        Mk, x, y, th, zx, zy = known_map_case(pop, n, L, K, q, s, q_lo=q * DETCOV_Q_LO)
        noise = detection_covs(K, s, q)
        per_k = list(zip(*noise))
        det = dets_detcov(np.broadcast_to(Mk, (n,) + Mk.shape), th, noise)
    return Mk, x, y, th, zx, zy, noise, per_k, det
