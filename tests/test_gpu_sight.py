"""slam_sight_table_dev and slam_landmark_evidence_sight_dev (csrc/sight_kernels.hip; csrc/evidence_kernels.hip: the one stage with line of sight) against their specification
tests/_sight_spec.py: the table bit for bit whatever the scan and the bins; map rows, evidence bytes, stats and spared counts bit
for bit whatever the shape, the gather index, the strides (the dword and the byte path) and the geometry; the scan hand-over drops
the table; the argument checks launch nothing."""
import numpy as np
import pytest
import torch

import _sight_spec as S
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
K, HIT, MISS, CMAX, RANGE, MARGIN = 4, 2, 1, 8, 9.0, 0.3
TINY = float(np.float32(1e-45))


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


def scan_of(nbeams, seed):
    """Points in every quadrant at 0.5 .. 6 m; from 8 beams on also the four axes, the origin, -0.0, a subnormal, an inf point."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-np.pi, np.pi, nbeams)
    r = rng.uniform(0.5, 6.0, nbeams)
    bx, by = (r * np.cos(a)).astype(F), (r * np.sin(a)).astype(F)
    special = [(2, 0), (0, 2), (-2, 0), (0, -2), (0, 0), (1.5, -0.0), (1.0, -TINY), (np.inf, 1.0), (-0.0, -3.0), (3e38, 3e38)]
    if nbeams >= 8:
        for k, (x, y) in enumerate(special[:nbeams // 2]):
            bx[2 * k], by[2 * k] = x, y
    return bx, by


@pytest.mark.parametrize("bins", [32, 128, 1024])
@pytest.mark.parametrize("nbeams", [1, 63, 360, 1081])
def test_table_equals_the_spec(eng, nbeams, bins):
    bx, by = scan_of(nbeams, 10 * nbeams + bins)
    c0 = eng.sight_counts()
    eng.scan_upload(bx, by)
    eng.sight_table_dev(bins)
    got, want = eng.sight_table(), S.table(bx, by, bins)
    assert got.shape == (bins,) and np.array_equal(bits(got), bits(want))
    assert np.isfinite(want).sum() >= min(nbeams, 1) and (nbeams < bins or np.isfinite(want).sum() > bins // 4)
    assert eng.sight_counts() == (c0[0] + 1, c0[1])
    # the same scan as device arrays, another bin count behind it: the whole buffer is rewritten
    d_bx, d_by = dev(bx), dev(by)
    eng.scan_set_dev(d_bx, d_by, nbeams)
    other = 64 if bins != 64 else 32
    eng.sight_table_dev(other)
    assert np.array_equal(bits(eng.sight_table()), bits(S.table(bx, by, other)))
    eng.scan_upload(bx, by)


def test_empty_scan_and_hand_over(eng):
    pkg = load_package()
    eng.scan_upload(np.zeros(0, F), np.zeros(0, F))
    eng.sight_table_dev(32)
    assert np.array_equal(eng.sight_table(), np.full(32, np.inf, F))
    for hand_over in (lambda: eng.scan_upload(np.ones(3, F), np.ones(3, F)), lambda: eng.scan_set_dev(dev(np.ones(3, F)), dev(np.ones(3, F)), 3)):
        eng.sight_table_dev(32)
        hand_over()                                                    # a new scan: the table of the old one is dropped
        with pytest.raises(pkg.SlamError) as err:
            eng.sight_table()
        assert err.value.status == -4


# ------------------------------------------------------------------ the stage
def make_case(n, L, plane_stride, rows, bins, seed, k_dets=K):
    """Poses, a scan (a ring of returns at 2 m over three quarters of the circle, open elsewhere), landmarks and their table bytes
    and evidence: every branch of the rule per particle.  Landmark l of particle i is placed in the SENSOR frame and moved to the
    world with float64 trigonometry (the rule then rotates it back in float32: near a bin edge either side is right, and the spec
    decides).  Roles by l mod 12 (shifted by i); landmark 0 / 1 of each particle lie in bins 0 / bins - 1."""
    rng = np.random.default_rng(seed)
    x, y = (rng.integers(-20, 20, n) / 4).astype(F), (rng.integers(-20, 20, n) / 4).astype(F)
    th = rng.uniform(-3.0, 3.0, n).astype(F)
    a = np.linspace(-np.pi, np.pi, 720, endpoint=False)
    a = a[(a < np.pi / 2)]                              # the second quadrant is open: nothing hides anything there
    bx, by = (2.0 * np.cos(a)).astype(F), (2.0 * np.sin(a)).astype(F)
    mp = (rng.standard_normal((n, 5, plane_stride)) * 1e3).astype(F)
    mp[rng.random(mp.shape) < 0.2] = np.nan
    mp[:, 2][rng.random((n, plane_stride)) < 0.3] = -1.0
    tab = np.full((n, L), 255, np.uint8)
    c = np.zeros((n, L), np.uint8)
    role = (np.arange(L)[None, :] + np.arange(n)[:, None]) % 12
    eps = 0.4 / bins                                    # well inside the first / the last bin
    for i in range(n):
        for l in range(L):
            ro = role[i, l]
            ang = rng.uniform(-np.pi, np.pi / 2 - 0.1)
            r, pxx, t, cc = 4.0, 0.3, 255, 0
            if L == 1:                                  # one landmark per particle: the particles share the roles out
                ro = (0, 1, 2, 8, 10)[i % 5]
                ang = (eps, -eps, ang, ang, ang)[i % 5]
            elif l == 0:
                ang, ro = eps, 0
            elif l == 1:
                ang, ro = -eps, 0
            if ro == 0:
                pass                                    # behind the ring, no hit, c = 0: SPARED (plain: pruned)
            elif ro == 1:
                t, cc = int(rng.integers(0, k_dets)) if k_dets else 255, 3      # behind the ring and HIT: the hit counts
            elif ro == 2:
                r = 1.0                                 # in front of the ring, c = 0: PRUNED
            elif ro == 3:
                r, cc = 1.5, 5                          # in front of the ring: a miss paid
            elif ro == 4:
                ang = rng.uniform(np.pi / 2 + 0.2, np.pi - 0.2)                  # the open quadrant: PRUNED
            elif ro == 5:
                r = 2.2                                 # behind the ring by less than the margin: not hidden, PRUNED
            elif ro == 6:
                pxx, t = -1.0, 0                        # unseen
            elif ro == 7:
                r, cc = 30.0, 4                         # out of range: stays
            elif ro == 8:
                r, cc = 0.0, 2                          # at the particle's position: no bin, g <= 0: a miss paid
            elif ro == 9:
                r, cc = 0.2, 0                          # nearer than the margin: PRUNED
            elif ro == 10:
                cc = 7                                  # behind the ring with evidence: spared, c stays
            elif ro == 11:
                r, t, cc = 1.0, K + 1, 1                # a byte that names no detection: no hit; a miss paid exactly
            zx, zy = r * np.cos(ang), r * np.sin(ang)
            co, si = np.cos(float(th[i])), np.sin(float(th[i]))
            mp[i, 0, l] = x[i] + co * zx + si * zy      # w = t + R(theta)^T z
            mp[i, 1, l] = y[i] - si * zx + co * zy
            if ro == 8:
                mp[i, 0, l], mp[i, 1, l] = x[i], y[i]
            mp[i, 2, l] = pxx
            tab[i, l], c[i, l] = t, cc
    if L >= 14:
        mp[0, 0, 13] = np.nan                           # a NaN mean: not visible, nothing happens to it
        mp[0, 2, 13], tab[0, 13], c[0, 13] = 0.3, 255, 6
    ev = rng.integers(0, 256, (rows, L)).astype(np.uint8)
    return (x, y, th), (bx, by), mp, tab, c, ev


def run_case(eng, n, L, plane_stride, ev_stride, assoc_stride, mode, bins, seed, offset=0, k_dets=K, label=""):
    rng = np.random.default_rng(seed + 1)
    rows = n + 3 if mode == "dup" else n
    # out of place: through repeated, out-of-order ancestors (L == 1: out of order only — every particle keeps the evidence of its role)
    anc = (rng.permutation(rows)[:n] if L == 1 else rng.integers(0, rows, n)).astype(np.int32) if mode == "dup" else None
    (x, y, th), (bx, by), mp, tab, c, ev = make_case(n, L, plane_stride, rows, bins, seed, k_dets)
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
    eng.sight_table_dev(bins)
    T = S.table(bx, by, bins)
    want_mp, want_ev, want_st, want_sp = S.evidence(mp, x, y, th, anc, body(h_tab, n, assoc_stride), k_dets, body(h_in, rows, ev_stride), HIT,
                                                    MISS, CMAX, RANGE, T, MARGIN, L=L, in_place=in_place)
    if in_place:
        h_out, d_out = h_in, d_in
    else:
        h_out, d_out = guarded(np.zeros((n, 0), np.uint8), ev_stride, fill=7)
    want_flat = h_out.copy()
    body(want_flat, n, ev_stride)[:] = want_ev
    d_mp = dev(mp)
    d_st = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
    d_sp = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    at = G + offset
    eng.landmark_evidence_sight_dev(d_mp, 5 * plane_stride, plane_stride, L, dev(x), dev(y), dev(th), dev(anc) if anc is not None else None, n,
                                    d_tab[at:], assoc_stride, d_in[at:], d_out[at:], ev_stride, HIT, MISS, CMAX, RANGE, MARGIN, d_st, d_sp)
    got_flat, got_mp, got_st, got_sp = host(d_out), host(d_mp), host(d_st), host(d_sp)
    assert np.array_equal(got_sp, want_sp), f"{label}: spared {got_sp.tolist()} != {want_sp.tolist()}"
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(got_flat, want_flat), f"{label}: evidence differs at {np.argwhere(got_flat != want_flat)[:5].ravel().tolist()}"
    assert np.array_equal(bits(got_mp), bits(want_mp)), f"{label}: map rows"
    assert np.array_equal(host(d_tab), h_tab), f"{label}: the table changed"
    if not in_place:
        assert np.array_equal(host(d_in), h_in), f"{label}: the source evidence changed"
    # what the case holds: a pruned, a spared and a hit-while-hidden landmark, and landmarks in the first and the last bin
    hid, j, has = S.hidden(T, MARGIN, x, y, th, mp[:n, 0, :L], mp[:n, 1, :L])
    seen = ~(mp[:n, 2, :L] < 0)
    hit_now = body(h_tab, n, assoc_stride)[:, :L] < k_dets
    return dict(pruned=int(want_st[:, 0].sum()), spared=int(want_sp.sum()), hidden_hit=int((hid & seen & hit_now).sum()),
                first=int(((j == 0) & has & hid).sum()), last=int(((j == bins - 1) & has & hid).sum()), no_bin=int((~has & seen).sum()))


def configs(L):
    """(plane_stride, ev_stride, assoc_stride, mode, offset): byte strides multiples of 4 (the dword path) and odd, or an odd base."""
    Lp, L4 = (L + 31) // 32 * 32, (L + 3) // 4 * 4
    odd = L + 1 if (L + 1) % 2 else L + 2
    return ((Lp, Lp, L4 + 4, "dup", 0), (Lp + 32, odd, odd + 2, "dup", 0), (Lp, L4, Lp, "inplace", 0), (Lp + 64, odd, L4, "inplace", 0),
            (Lp, L4 + 8, L4, "dup", 1), (Lp, L4, L4 + 4, "inplace", 1))


@pytest.mark.parametrize("L", [1, 64, 65, 128, 129, 200])
def test_stage_equals_the_spec(eng, L):
    n = 5
    for j, (ps, es, ts, mode, offset) in enumerate(configs(L)):
        bins = (32, 128, 1024)[j % 3]
        got = run_case(eng, n, L, ps, es, ts, mode, bins, seed=100 * L + j, offset=offset, label=f"L={L} config {j} bins {bins}")
        # every launch holds a pruned, a spared and a hit-while-hidden landmark, hidden ones in the first and the last bin (the
        # neighbour window wraps), and one without a bin
        assert all(v > 0 for v in got.values()), (j, got)


def test_two_landmarks_and_several_workgroups(eng):
    """L = 2 (bins 0 and bins - 1 only) and L = 13 with a particle count that is no multiple of a workgroup's four, over 64 workgroups."""
    got = run_case(eng, 5, 2, 32, 4, 4, "dup", 128, seed=7, label="L=2")
    assert got["first"] > 0 and got["last"] > 0 and got["spared"] == 10
    got = run_case(eng, 259, 13, 32, 16, 16, "dup", 64, seed=8, label="n=259")
    assert got["pruned"] > 0 and got["spared"] > 0 and got["hidden_hit"] > 0
    got = run_case(eng, 259, 13, 32, 15, 13, "inplace", 64, seed=9, label="n=259 bytes")
    assert got["pruned"] > 0 and got["spared"] > 0


def test_no_detections(eng):
    try:
        eng.detections_upload(np.zeros(0, F), np.zeros(0, F))
        got = run_case(eng, 5, 65, 96, 68, 68, "dup", 128, seed=3, k_dets=0, label="K = 0")
        assert got["pruned"] > 0 and got["spared"] > 0 and got["hidden_hit"] == 0
        run_case(eng, 5, 65, 96, 67, 69, "inplace", 128, seed=4, k_dets=0, label="K = 0 in place")
    finally:
        eng.detections_upload(np.zeros(K, F), np.zeros(K, F))


def test_argument_checks_and_counters(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    (x, y, th), (bx, by), mp, tab, c, _ = make_case(n, L, Lp, n, 128, 3)
    d_mp, d_x, d_y, d_th = dev(mp), dev(x), dev(y), dev(th)
    d_tab = torch.full((n, Lp), 255, dtype=torch.uint8, device=DEV)
    d_in = torch.full((n, Lp), 5, dtype=torch.uint8, device=DEV)
    d_out = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    d_sp = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    d_anc = dev(np.zeros(n, np.int32))
    ok = dict(mp=d_mp, ps=Lp, L=L, x=d_x, y=d_y, th=d_th, anc=None, tab=d_tab, ts=Lp, ein=d_in, eout=d_out, es=Lp, hit=1, miss=1, cmax=8,
              vr=5.0, mg=0.3)

    def call(e, **change):
        a = dict(ok, **change)
        e.landmark_evidence_sight_dev(a["mp"], 5 * a["ps"], a["ps"], a["L"], a["x"], a["y"], a["th"], a["anc"], n, a["tab"], a["ts"], a["ein"],
                                      a["eout"], a["es"], a["hit"], a["miss"], a["cmax"], a["vr"], a["mg"], None, d_sp)

    fresh = pkg.Engine(0)
    with pytest.raises(pkg.SlamError) as err:                       # no scan
        fresh.sight_table_dev(128)
    assert err.value.status == -4
    with pytest.raises(pkg.SlamError) as err:                       # no table to read back
        fresh.sight_table()
    assert err.value.status == -4
    fresh.scan_upload(bx, by)
    for bad in (0, 16, 31, 33, 96, 2048, -128):
        with pytest.raises(pkg.SlamError) as err:
            fresh.sight_table_dev(bad)
        assert err.value.status == -2, bad
    fresh.sight_table_dev(128)
    with pytest.raises(pkg.SlamError) as err:                       # a table, but no detections handed over
        call(fresh)
    assert err.value.status == -4
    fresh.detections_upload(np.zeros(K, F), np.zeros(K, F))
    fresh.scan_upload(bx, by)                                       # detections, but the table went with the old scan
    with pytest.raises(pkg.SlamError) as err:
        call(fresh)
    assert err.value.status == -4 and fresh.sight_counts() == (1, 0) and fresh.evidence_counts() == (0, 0)
    fresh.close()
    eng.scan_upload(bx, by)
    eng.sight_table_dev(128)
    c0, v0 = eng.sight_counts(), eng.evidence_counts()
    for change in (dict(hit=0), dict(hit=256), dict(hit=-1), dict(miss=0), dict(miss=256), dict(cmax=0), dict(cmax=256),
                   dict(vr=0.0), dict(vr=-1.0), dict(vr=float("nan")), dict(vr=float("inf")), dict(mg=0.0), dict(mg=-0.3), dict(mg=float("nan")),
                   dict(mg=float("inf")), dict(L=8193, ps=8200, ts=8200, es=8200), dict(ts=L - 1), dict(es=L - 1), dict(ps=L - 1),
                   dict(anc=d_anc, eout=d_in), dict(mp=None), dict(x=None), dict(y=None), dict(th=None), dict(tab=None), dict(ein=None),
                   dict(eout=None)):
        with pytest.raises(pkg.SlamError) as err:
            call(eng, **change)
        assert err.value.status == -2, change
    # nothing was launched
    assert eng.sight_counts() == c0 and np.all(host(d_out) == 7) and np.all(host(d_in) == 5) and np.all(host(d_sp) == -1)
    assert np.array_equal(bits(host(d_mp)), bits(mp))
    call(eng)                                                       # (no stats wanted)
    call(eng, anc=d_anc)
    eng.sync()
    assert eng.sight_counts() == (c0[0], c0[1] + 2) and eng.evidence_counts() == v0
