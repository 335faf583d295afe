"""slam_landmark_evidence_fov_dev (the evidence stage of csrc/evidence_kernels.hip with its field of view) against its specification tests/_fov_spec.py: map rows, evidence bytes,
stats, spared and outside counts bit for bit whatever the shape, the gather index, the strides (the dword and the byte path), the
arc (ordinary, wrapping, the reference sensor's) and line of sight on or off; landmarks exactly on a bound; with everything in
view the outputs of the stages it stands in for; the argument checks launch nothing."""
import numpy as np
import pytest
import torch

import _assoc_weight_spec as W
import _evidence_spec as E
import _fov_spec as V
import _sight_spec as S
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
K, HIT, MISS, CMAX, RANGE, MARGIN = 4, 2, 1, 8, 9.0, 0.3
ANGLES = -2.351831 + 0.004363 * np.arange(1079)
DEG = np.pi / 180
# (lo, hi), and in true sensor-frame angles: where a landmark is in view behind the scan's ring, where it is outside the arc
ARCS = {
    "ordinary": ((F(0.5), F(2.5)), (48 * DEG, 84 * DEG), (-132 * DEG, 42 * DEG)),
    "wrapping": ((F(2.5), F(1.5)), (-132 * DEG, 84 * DEG), (138 * DEG, 222 * DEG)),
    "sensor": ((V.bound(F(ANGLES[0]) + F(0.1)), V.bound(F(ANGLES[-1]) - F(0.1))), (-126 * DEG, 84 * DEG), (132 * DEG, 228 * DEG)),
}


# L <= 2: the roles of the landmarks of particle i % 5 (None: the particle whose landmarks lie on the bounds) — outside, spared,
# pruned and hit while outside in every launch
SMALL = {1: ((4,), (0,), (2,), (9,), None), 2: (None, (4, 0), (2, 9), (10, 5), (1, 3))}


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    e.detections_upload(np.zeros(K, F), np.zeros(K, F))
    yield e
    torch.cuda.synchronize()
    e.close()


def on_bound(p):
    """A sensor-frame point (|zx| a small integer) whose diamond angle is exactly p."""
    p = F(p)
    quad = min(int(p), 3)
    q = float((p, F(2) - p, p - F(2), F(4) - p)[quad])
    sx, sy = ((1, 1), (-1, 1), (-1, -1), (1, -1))[quad]
    for ax in range(1, 64):
        ay = F(ax * q / (1 - q))
        for cand in [ay] + [f(ay, k) for k in range(1, 40) for f in (lambda a, k: a + k * np.spacing(a), lambda a, k: a - k * np.spacing(a))]:
            zx, zy = F(sx * ax), F(sy * F(cand))
            if V.diamond(zx, zy)[0] == p:
                return float(zx), float(zy)
    raise AssertionError(f"no float32 point with diamond angle {p!r}")


def make_case(n, L, plane_stride, rows, arc, seed, k_dets=K):
    """Poses, the scan of test_gpu_sight.py (a ring of returns at 2 m over three quarters of the circle, open in the second
    quadrant), landmarks and their table bytes and evidence: every branch of the rule per particle.  Landmark l of particle i is
    placed in the SENSOR frame and moved to the world with float64 trigonometry.  Roles by l mod 12 (shifted by i); L <= 2: the five
    particles share the roles out (SMALL).  The particles with i % 7 == 0 (L == 1: particle 4) stand at an integer position with
    th = 0: their landmarks 0 / 1 lie EXACTLY on lo / hi and 2 / 3 just beyond them."""
    (lo, hi), behind, outside = ARCS[arc]
    rng = np.random.default_rng(seed)
    x, y = (rng.integers(-20, 20, n) / 4).astype(F), (rng.integers(-20, 20, n) / 4).astype(F)
    th = rng.uniform(-3.0, 3.0, n).astype(F)
    a = np.linspace(-np.pi, np.pi, 720, endpoint=False)
    a = a[(a < np.pi / 2)]
    bx, by = (2.0 * np.cos(a)).astype(F), (2.0 * np.sin(a)).astype(F)
    mp = (rng.standard_normal((n, 5, plane_stride)) * 1e3).astype(F)
    mp[rng.random(mp.shape) < 0.2] = np.nan
    mp[:, 2][rng.random((n, plane_stride)) < 0.3] = -1.0
    tab = np.full((n, L), 255, np.uint8)
    c = np.zeros((n, L), np.uint8)
    role = (np.arange(L)[None, :] + np.arange(n)[:, None]) % 12
    exact = np.zeros((n, L), np.int8)                   # 1: exactly on lo, 2: exactly on hi
    edge_pts = []
    for p in (lo, hi):
        zx, zy = on_bound(p)
        beyond = [(zx, zy + d) for d in (0.01, -0.01) if not V.in_view(*V.diamond(F(zx), F(zy + d)), lo, hi)]
        edge_pts.append(((zx, zy), beyond[0]))
    for i in range(n):
        small = SMALL[L][i % 5] if L <= 2 else ()
        special = small is None if L <= 2 else (i % 7 == 0)
        if special:
            x[i], y[i], th[i] = float(i % 5 - 2), 0.0, 0.0
        for l in range(L):
            ro = role[i, l]
            if small:
                ro = small[l]
            ang = rng.uniform(*behind)
            r, pxx, t, cc = 4.0, 0.3, 255, 0
            if ro == 0:
                pass                                    # in view behind the ring, no hit, c = 0: sight SPARED, plain PRUNED
            elif ro == 1:
                t, cc = int(rng.integers(0, k_dets)) if k_dets else 255, 3      # in view and HIT
            elif ro == 2:
                r = 1.0                                 # in view in front of the ring, c = 0: PRUNED
            elif ro == 3:
                r, cc = 1.5, 5                          # in view in front of the ring: a miss paid
            elif ro == 4:
                ang = rng.uniform(*outside)             # OUTSIDE, c = 0: the counter stays, the slot too
            elif ro == 5:
                ang, r, cc = rng.uniform(*outside), 1.0, 5   # OUTSIDE in front of the ring: c stays
            elif ro == 6:
                pxx, t = -1.0, 0                        # unseen
            elif ro == 7:
                ang, r, cc = rng.uniform(*outside), 30.0, 4  # outside and out of range: not due, not counted
            elif ro == 8:
                r, cc = 0.0, 2                          # at the particle's position: no bin, in view: a miss paid
            elif ro == 9:
                ang, t, cc = rng.uniform(*outside), int(rng.integers(0, k_dets)) if k_dets else 255, 3   # OUTSIDE and HIT: the hit counts
            elif ro == 10:
                cc = 7                                  # in view behind the ring with evidence: sight spared, plain a miss paid
            elif ro == 11:
                r, t, cc = 1.0, K + 1, 1                # a byte that names no detection: no hit; a miss paid exactly
            zx, zy = r * np.cos(ang), r * np.sin(ang)
            if special and l < 4:                       # th = 0, y = 0, x an integer: x + zx and zy are exact
                (zx, zy), t, cc, pxx = edge_pts[l % 2][l // 2], 255, 5, 0.3
                exact[i, l] = (1, 2, 0, 0)[l]
                ro = -1
            co, si = np.cos(float(th[i])), np.sin(float(th[i]))
            mp[i, 0, l] = x[i] + co * zx + si * zy      # w = t + R(theta)^T z
            mp[i, 1, l] = y[i] - si * zx + co * zy
            if ro == 8:
                mp[i, 0, l], mp[i, 1, l] = x[i], y[i]
            mp[i, 2, l] = pxx
            tab[i, l], c[i, l] = t, cc
    if L >= 14:
        mp[1, 0, 13] = np.nan                           # a NaN mean: not visible, nothing happens to it
        mp[1, 2, 13], tab[1, 13], c[1, 13] = 0.3, 255, 6
    ev = rng.integers(0, 256, (rows, L)).astype(np.uint8)
    return (x, y, th), (bx, by), mp, tab, c, ev, exact


def run_case(eng, n, L, plane_stride, ev_stride, assoc_stride, mode, arc, bins, seed, offset=0, k_dets=K, label="", bounds=None, parent=False):
    """bins = 0: without line of sight.  bounds: instead of the arc's.  parent: also run the stage this one stands in for on the same
    inputs and return both outputs."""
    rng = np.random.default_rng(seed + 1)
    rows = n + 3 if mode == "dup" else n
    anc = (rng.permutation(rows)[:n] if L <= 2 else rng.integers(0, rows, n)).astype(np.int32) if mode == "dup" else None
    (x, y, th), (bx, by), mp, tab, c, ev, exact = make_case(n, L, plane_stride, rows, arc, seed, k_dets)
    lo, hi = bounds or ARCS[arc][0]
    src = np.arange(n) if anc is None else anc
    if mode == "dup":                                   # several particles may read one row: all of them then see the last writer's bytes
        for i in range(n):
            ev[src[i]] = c[i]
    else:
        ev[src] = c
    G = 16
    def guarded(arr, stride, fill=None, s=0):
        r_, l_ = arr.shape
        flat = np.random.default_rng(seed + s).integers(0, 256, 2 * G + offset + r_ * stride).astype(np.uint8) if fill is None else \
            np.full(2 * G + offset + r_ * stride, fill, np.uint8)
        flat[G + offset:G + offset + r_ * stride].reshape(r_, stride)[:, :l_] = arr
        return flat, dev(flat)
    body = lambda flat, r_, stride: flat[G + offset:G + offset + r_ * stride].reshape(r_, stride)
    h_tab, d_tab = guarded(tab, assoc_stride, s=2)
    h_in, d_in = guarded(ev, ev_stride, s=3)
    in_place = mode == "inplace"
    eng.scan_upload(bx, by)
    T = None
    if bins:
        eng.sight_table_dev(bins)
        T = S.table(bx, by, bins)
    want_mp, want_ev, want_st, want_sp, want_out = V.evidence(mp, x, y, th, anc, body(h_tab, n, assoc_stride), k_dets, body(h_in, rows, ev_stride),
                                                              HIT, MISS, CMAX, RANGE, lo, hi, T, MARGIN if bins else None, L=L, in_place=in_place)
    at = G + offset
    outs = []
    for which in (("fov", "parent") if parent else ("fov",)):
        d_in_k = d_in.clone()
        if in_place:
            h_out, d_out = h_in, d_in_k
        else:
            h_out, d_out = guarded(np.zeros((n, 0), np.uint8), ev_stride, fill=7)
        d_mp = dev(mp)
        d_st = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
        d_sp = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        d_ou = torch.full((n,), -1, dtype=torch.int32, device=DEV)
        head = (d_mp, 5 * plane_stride, plane_stride, L, dev(x), dev(y))
        mid = (dev(anc) if anc is not None else None, n, d_tab[at:], assoc_stride, d_in_k[at:], d_out[at:], ev_stride, HIT, MISS, CMAX, RANGE)
        if which == "fov":
            eng.landmark_evidence_fov_dev(*head, dev(th), *mid, MARGIN, float(lo), float(hi), bool(bins), d_st, d_sp, d_ou)
        elif bins:
            eng.landmark_evidence_sight_dev(*head, dev(th), *mid, MARGIN, d_st, d_sp)
        else:
            eng.landmark_evidence_dev(*head, *mid, d_st)
        outs.append(dict(flat=host(d_out), mp=host(d_mp), st=host(d_st), sp=host(d_sp), ou=host(d_ou), src=host(d_in_k)))
    got = outs[0]
    want_flat = h_out.copy()
    body(want_flat, n, ev_stride)[:] = want_ev
    assert np.array_equal(got["ou"], want_out), f"{label}: outside {got['ou'].tolist()} != {want_out.tolist()}"
    assert np.array_equal(got["sp"], want_sp), f"{label}: spared {got['sp'].tolist()} != {want_sp.tolist()}"
    assert np.array_equal(got["st"], want_st), f"{label}: stats"
    assert np.array_equal(got["flat"], want_flat), f"{label}: evidence differs at {np.argwhere(got['flat'] != want_flat)[:5].ravel().tolist()}"
    assert np.array_equal(bits(got["mp"]), bits(want_mp)), f"{label}: map rows"
    assert np.array_equal(host(d_tab), h_tab), f"{label}: the table changed"
    if not in_place:
        assert np.array_equal(got["src"], h_in), f"{label}: the source evidence changed"
    if parent:
        return outs
    # what the case holds, by the spec
    zx, zy = V.sensor_frame(x, y, th, mp[:n, 0, :L], mp[:n, 1, :L])
    p, has = V.diamond(zx, zy)
    view = V.in_view(p, has, lo, hi)
    seen = ~(mp[:n, 2, :L] < 0)
    hit_now = body(h_tab, n, assoc_stride)[:, :L] < k_dets
    on_lo, on_hi = (exact == 1) & has & (p == lo), (exact == 2) & has & (p == hi)
    assert on_lo.sum() == (exact == 1).sum() and on_hi.sum() == (exact == 2).sum(), f"{label}: the landmarks meant to lie on a bound do not"
    assert view[on_lo].all() and view[on_hi].all(), f"{label}: a landmark on a bound is not in view"
    return dict(outside=int(want_out.sum()), spared=int(want_sp.sum()), pruned=int(want_st[:, 0].sum()),
                outside_hit=int((~view & seen & hit_now).sum()), on_lo=int(on_lo.sum()), on_hi=int(on_hi.sum()), no_bin=int((~has & seen).sum()))


def configs(L):
    """(plane_stride, ev_stride, assoc_stride, mode, offset): byte strides multiples of 4 (the dword path) and odd, or an odd base."""
    Lp, L4 = (L + 31) // 32 * 32, (L + 3) // 4 * 4
    odd = L + 1 if (L + 1) % 2 else L + 2
    return ((Lp, Lp, L4 + 4, "dup", 0), (Lp + 32, odd, odd + 2, "dup", 0), (Lp, L4, Lp, "inplace", 0), (Lp + 64, odd, L4, "inplace", 0),
            (Lp, L4 + 8, L4, "dup", 1), (Lp, L4, L4 + 4, "inplace", 1))


def holds_every_kind(got, L, sight):
    kinds = ["outside", "pruned", "outside_hit"] + (["spared"] if sight else [])
    kinds += ["on_lo", "on_hi", "no_bin"] if L >= 12 else (["on_lo", "on_hi"] if L >= 2 else ["on_lo"])
    return all(got[k] > 0 for k in kinds)


@pytest.mark.parametrize("L", [1, 2, 64, 65, 128, 129, 200])
def test_stage_equals_the_spec(eng, L):
    n = 5
    c0, s0, v0 = eng.fov_counts(), eng.sight_counts(), eng.evidence_counts()
    launches = tables = 0
    for j, (ps, es, ts, mode, offset) in enumerate(configs(L)):
        for k, arc in enumerate(ARCS):
            bins = (0, 32, 128, 1024)[(j + k) % 4]
            got = run_case(eng, n, L, ps, es, ts, mode, arc, bins, seed=100 * L + 10 * j + k, offset=offset,
                           label=f"L={L} config {j} {arc} bins {bins}")
            launches, tables = launches + 1, tables + (bins != 0)
            assert holds_every_kind(got, L, bins != 0) and got["on_lo"] > 0, (j, arc, bins, got)
    # the stage counts here and in no other counter; a table counts where it always did
    assert eng.fov_counts() == c0 + launches and eng.sight_counts() == (s0[0] + tables, s0[1]) and eng.evidence_counts() == v0


def test_several_workgroups(eng):
    """L = 13 with a particle count that is no multiple of a workgroup's four, over 64 workgroups: the dword and the byte path."""
    for j, (es, ts, mode, arc, bins) in enumerate(((16, 16, "dup", "sensor", 64), (15, 13, "inplace", "sensor", 0), (16, 16, "inplace", "ordinary", 1024),
                                                   (13, 17, "dup", "wrapping", 0))):
        got = run_case(eng, 259, 13, 32, es, ts, mode, arc, bins, seed=8 + j, label=f"n=259 {j}")
        assert holds_every_kind(got, 13, bins != 0), got


def test_no_detections(eng):
    try:
        eng.detections_upload(np.zeros(0, F), np.zeros(0, F))
        got = run_case(eng, 5, 65, 96, 68, 68, "dup", "sensor", 128, seed=3, k_dets=0, label="K = 0")
        assert got["pruned"] > 0 and got["spared"] > 0 and got["outside"] > 0 and got["outside_hit"] == 0
        run_case(eng, 5, 65, 96, 67, 69, "inplace", "wrapping", 0, seed=4, k_dets=0, label="K = 0 in place")
    finally:
        eng.detections_upload(np.zeros(K, F), np.zeros(K, F))


@pytest.mark.parametrize("bins", [0, 128])
def test_everything_in_view_is_the_stage_it_stands_in_for(eng, bins):
    for L, (ps, es, ts, mode, offset) in ((65, configs(65)[0]), (129, configs(129)[3]), (13, configs(13)[4])):
        fov, parent = run_case(eng, 7, L, ps, es, ts, mode, "sensor", bins, seed=50 + L, offset=offset, bounds=V.ALL, parent=True,
                               label=f"all in view L={L} bins {bins}")
        assert fov["st"][:, 0].sum() > 0 and np.all(fov["ou"] == 0) and np.all(parent["ou"] == -1)
        for k in ("flat", "mp", "st", "src"):
            assert fov[k].tobytes() == parent[k].tobytes(), (L, k)
        if bins:
            assert np.array_equal(fov["sp"], parent["sp"]) and fov["sp"].sum() > 0
        else:
            assert np.all(fov["sp"] == 0)


def test_six_entry_points_side_by_side(eng):
    """The stage is one path behind six entry points: per form the call with the miss count and the one without write the same
    bytes, the count is the specification's, and each call moves its own launch counter and no other."""
    n, BINS = 7, 128
    lo, hi = ARCS["sensor"][0]
    for L in (13, 65, 129):
        for j in (0, 1):                                # the dword path, the byte path (odd strides); both through ancestors
            ps, es, ts, _, _ = configs(L)[j]
            rows = n + 3
            rng = np.random.default_rng(900 + 10 * L + j)
            anc = rng.permutation(rows)[:n].astype(np.int32)
            (x, y, th), (bx, by), mp, tab, c, ev, _ = make_case(n, L, ps, rows, "sensor", seed=60 + L + j)
            ev[anc] = c
            h_in = rng.integers(0, 256, (rows, es)).astype(np.uint8)
            h_in[:, :L] = ev
            h_tab = rng.integers(0, 256, (n, ts)).astype(np.uint8)
            h_tab[:, :L] = tab
            eng.scan_upload(bx, by)
            eng.sight_table_dev(BINS)
            T = S.table(bx, by, BINS)
            spec = {"plain": E.evidence(mp, x, y, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, L=L),
                    "sight": S.evidence(mp, x, y, th, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, T, MARGIN, L=L),
                    "fov": V.evidence(mp, x, y, th, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, lo, hi, T, MARGIN, L=L)}
            # which of (evidence stage, sight stage, fov stage) launches a form counts in
            for form, moves in (("plain", (1, 0, 0)), ("sight", (0, 1, 0)), ("fov", (0, 0, 1))):
                w_mp, w_ev, w_st = spec[form][:3]
                want = W.missed_of(h_in, anc, w_ev, mp, w_mp, L)
                outs = []
                for with_missed in (False, True):
                    d_mp, d_in, d_tab = dev(mp), dev(h_in), dev(h_tab)
                    d_out = torch.full((n, es), 7, dtype=torch.uint8, device=DEV)
                    d_st = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
                    d_sp, d_ou, d_ms = (torch.full((n,), -1, dtype=torch.int32, device=DEV) for _ in range(3))
                    head = (d_mp, 5 * ps, ps, L, dev(x), dev(y))
                    mid = (dev(anc), n, d_tab, ts, d_in, d_out, es, HIT, MISS, CMAX, RANGE)
                    ms = dict(d_missed=d_ms) if with_missed else {}
                    before = (eng.evidence_counts()[0], eng.sight_counts()[1], eng.fov_counts())
                    tables = (eng.evidence_counts()[1], eng.sight_counts()[0])
                    if form == "plain":
                        eng.landmark_evidence_dev(*head, *mid, d_st, **ms)
                    elif form == "sight":
                        eng.landmark_evidence_sight_dev(*head, dev(th), *mid, MARGIN, d_st, d_sp, **ms)
                    else:
                        eng.landmark_evidence_fov_dev(*head, dev(th), *mid, MARGIN, float(lo), float(hi), True, d_st, d_sp, d_ou, **ms)
                    after = (eng.evidence_counts()[0], eng.sight_counts()[1], eng.fov_counts())
                    label = f"L={L} config {j} {form} missed={with_missed}"
                    assert tuple(a - b for a, b in zip(after, before)) == moves, f"{label}: counters moved by {before} -> {after}"
                    assert (eng.evidence_counts()[1], eng.sight_counts()[0]) == tables, f"{label}: an init or table counter moved"
                    outs.append(tuple(host(t) for t in (d_mp, d_out, d_st, d_sp, d_ou, d_ms)))
                without, with_ = outs
                label = f"L={L} config {j} {form}"
                for a, b, what in zip(without[:5], with_[:5], ("map rows", "evidence", "stats", "spared", "outside")):
                    assert a.tobytes() == b.tobytes(), f"{label}: {what} differ between the call with the miss count and the one without"
                assert np.all(without[5] == -1) and np.array_equal(with_[5], want), f"{label}: missed {with_[5].tolist()} != {want.tolist()}"
                assert want.sum() > 0, f"{label}: the case holds no miss"
                # ... and they are the specification's
                assert np.array_equal(bits(with_[0]), bits(w_mp)) and np.array_equal(with_[1][:, :L], w_ev[:, :L]) and np.all(with_[1][:, L:] == 0)
                assert np.array_equal(with_[2], w_st), f"{label}: stats"
                assert np.array_equal(with_[3], spec[form][3] if form != "plain" else np.full(n, -1)), f"{label}: spared"
                assert np.array_equal(with_[4], spec[form][4] if form == "fov" else np.full(n, -1)), f"{label}: outside"


def test_argument_checks_and_counters(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    (x, y, th), (bx, by), mp, tab, c, _, _ = make_case(n, L, Lp, n, "sensor", 3)
    d_mp, d_x, d_y, d_th = dev(mp), dev(x), dev(y), dev(th)
    d_tab = torch.full((n, Lp), 255, dtype=torch.uint8, device=DEV)
    d_in = torch.full((n, Lp), 5, dtype=torch.uint8, device=DEV)
    d_out = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    d_sp = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_ou = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_anc = dev(np.zeros(n, np.int32))
    ok = dict(mp=d_mp, ps=Lp, L=L, x=d_x, y=d_y, th=d_th, anc=None, tab=d_tab, ts=Lp, ein=d_in, eout=d_out, es=Lp, hit=1, miss=1, cmax=8,
              vr=5.0, mg=0.3, lo=2.5, hi=1.5, sight=1)

    def call(e, **change):
        a = dict(ok, **change)
        e.landmark_evidence_fov_dev(a["mp"], 5 * a["ps"], a["ps"], a["L"], a["x"], a["y"], a["th"], a["anc"], n, a["tab"], a["ts"], a["ein"],
                                    a["eout"], a["es"], a["hit"], a["miss"], a["cmax"], a["vr"], a["mg"], a["lo"], a["hi"], a["sight"], None,
                                    d_sp, d_ou)

    fresh = pkg.Engine(0)
    fresh.scan_upload(bx, by)
    with pytest.raises(pkg.SlamError) as err:                       # no detections handed over
        call(fresh, sight=0)
    assert err.value.status == -4
    fresh.detections_upload(np.zeros(K, F), np.zeros(K, F))
    with pytest.raises(pkg.SlamError) as err:                       # detections, but no table: refused only with line of sight
        call(fresh)
    assert err.value.status == -4 and fresh.fov_counts() == 0
    call(fresh, sight=0, mg=float("nan"))                           # ... without it no table is needed and the margin is not read
    fresh.sync()
    assert fresh.fov_counts() == 1 and fresh.sight_counts() == (0, 0) and fresh.evidence_counts() == (0, 0)
    assert np.all(host(d_sp) == 0) and host(d_ou).min() >= 0        # spared is written 0
    fresh.close()
    d_out.fill_(7)
    d_in.fill_(5)
    d_sp.fill_(-1)
    d_ou.fill_(-1)
    d_mp.copy_(dev(mp))
    eng.scan_upload(bx, by)
    eng.sight_table_dev(128)
    c0, s0, v0 = eng.fov_counts(), eng.sight_counts(), eng.evidence_counts()
    nan, inf = float("nan"), float("inf")
    for change in (dict(hit=0), dict(hit=256), dict(hit=-1), dict(miss=0), dict(miss=256), dict(cmax=0), dict(cmax=256),
                   dict(vr=0.0), dict(vr=-1.0), dict(vr=nan), dict(vr=inf), dict(mg=0.0), dict(mg=-0.3), dict(mg=nan), dict(mg=inf),
                   dict(lo=nan), dict(hi=nan), dict(lo=-0.001), dict(hi=4.001), dict(lo=4.5), dict(hi=-1.0), dict(lo=inf), dict(hi=-inf),
                   dict(lo=nan, sight=0), dict(hi=5.0, sight=0),
                   dict(L=8193, ps=8200, ts=8200, es=8200), dict(ts=L - 1), dict(es=L - 1), dict(ps=L - 1),
                   dict(anc=d_anc, eout=d_in), dict(mp=None), dict(x=None), dict(y=None), dict(th=None), dict(th=None, sight=0), dict(tab=None),
                   dict(ein=None), dict(eout=None)):
        with pytest.raises(pkg.SlamError) as err:
            call(eng, **change)
        assert err.value.status == -2, change
    # nothing was launched
    assert eng.fov_counts() == c0 and np.all(host(d_out) == 7) and np.all(host(d_in) == 5) and np.all(host(d_sp) == -1) and np.all(host(d_ou) == -1)
    assert np.array_equal(bits(host(d_mp)), bits(mp))
    call(eng)                                                       # (no stats wanted)
    call(eng, anc=d_anc)
    call(eng, lo=0.0, hi=4.0, sight=0)                              # the bounds of the range are bounds
    eng.sync()
    assert eng.fov_counts() == c0 + 3 and eng.sight_counts() == s0 and eng.evidence_counts() == v0
