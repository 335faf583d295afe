"""slam_landmark_evidence_dev and slam_evidence_init_dev (csrc/evidence_kernels.hip: the one stage with neither switch on) against their specification
tests/_evidence_spec.py: map rows, evidence bytes and stats are equal bit for bit, whatever the shape, the gather index, the
strides and the alignment of the byte arrays (the dword and the byte path); nothing outside what the rule names is written; the
argument checks and the counters."""
import numpy as np
import pytest
import torch

import _evidence_spec as E
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
NS = (1, 3, 4, 5, 257)          # a wavefront, the workgroup's four, one over, several workgroups with a tail
LS = (1, 63, 64, 65, 127, 128, 129, 500)
K, HIT, MISS, CMAX, RANGE = 8, 3, 2, 9, 5.0
GUARD = 16                      # bytes in front of and behind every byte array, checked after each launch
UP3 = float(np.nextafter(F(3.0), F(4.0)))
# (mean, P_xx, table byte, evidence) per landmark, dealt out cyclically: every branch of the rule and the edges of
# test_evidence_spec_cpu.py.  mean: the offset from the particle's pose (poses are multiples of 1/4: the offsets survive exactly)
SCENARIOS = (
    ((1.0, 1.0), -1.0, 0, 5),                  # unseen: 0 whatever the table says
    ((1.0, -2.0), 0.3, 1, CMAX - 1),           # hit, clamped at cmax
    ((0.5, 0.25), 0.3, K - 1, 0),              # hit
    ((1.0, 1.0), 0.3, K + 1, MISS - 1),        # a byte K <= a < 64 is no hit; c == miss - 1: pruned
    ((-2.0, 1.0), 0.3, 200, MISS),             # a byte in 64 .. 254; c == miss: 0, not pruned
    ((1.0, 1.0), 0.3, 255, CMAX),              # a miss
    ((30.0, 1.0), 0.3, 255, 4),                # out of range: stays
    ((3.0, 4.0), 0.3, 255, MISS - 1),          # r2 == range2: visible, pruned
    ((UP3, 4.0), 0.3, 255, MISS - 1),          # the next float32: not visible
    ((np.nan, 1.0), 0.3, 255, MISS - 1),       # a NaN mean is not visible
    ((1.0, np.nan), 0.3, 2, 1),                # ... and a hit does not ask
    ((1.0, 1.0), -0.0, 255, 0),                # -0.0 counts as seen: pruned
    ((np.inf, 1.0), 0.3, 255, 3),              # an infinite mean
    ((40.0, -40.0), 0.3, 0, CMAX),             # hit out of range, already at cmax
    ((1.0, 1.0), np.nan, 255, MISS + 1),       # NaN P_xx: seen
    ((-3.0, -4.0), 0.3, K, CMAX),              # a == K exactly: no hit, r2 == range2: a miss
)


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)   # one stream for torch's fills and copies and the engine's launches
    e.detections_upload(np.zeros(K, F), np.zeros(K, F))
    yield e
    torch.cuda.synchronize()
    e.close()


def make_case(n, L, plane_stride, rows, variant, seed, params=(HIT, MISS, CMAX)):
    """-> (x, y [n], map [n][5][plane_stride], table bytes [n][L], evidence [rows][L]): scenario (i * L + l + variant) mod 16 for
    landmark l of particle i; the map's padding holds junk (NaN, negative P_xx), the evidence of rows no particle reads too."""
    rng = np.random.default_rng(seed)
    x = (rng.integers(-200, 200, n) / 4).astype(np.float32)
    y = (rng.integers(-200, 200, n) / 4).astype(np.float32)
    mp = (rng.standard_normal((n, 5, plane_stride)) * 1e3).astype(np.float32)
    mp[rng.random(mp.shape) < 0.2] = np.nan
    mp[:, 2][rng.random((n, plane_stride)) < 0.3] = -1.0
    s = (np.arange(n)[:, None] * L + np.arange(L)[None, :] + variant) % len(SCENARIOS)
    off = np.array([sc[0] for sc in SCENARIOS], np.float32)
    mp[:, 0, :L] = x[:, None] + off[s, 0]
    mp[:, 1, :L] = y[:, None] + off[s, 1]
    mp[:, 2, :L] = np.array([sc[1] for sc in SCENARIOS], np.float32)[s]
    tab = np.array([sc[2] for sc in SCENARIOS], np.uint8)[s]
    c = np.array([sc[3] for sc in SCENARIOS], np.uint8)[s]
    if params != (HIT, MISS, CMAX):   # other parameters: any evidence, the scenarios' geometry and table bytes
        c = rng.integers(0, 256, (n, L)).astype(np.uint8)
    ev = rng.integers(0, 256, (rows, L)).astype(np.uint8)
    return x, y, mp, tab, c, ev


def guarded(a, stride, offset=0, fill=None, seed=0):
    """A [rows][L] byte array -> flat device buffer GUARD | offset | rows x stride | GUARD with random padding columns, and the
    same on the host; the array proper starts at byte GUARD + offset."""
    rows, L = a.shape
    rng = np.random.default_rng(seed)
    flat = rng.integers(0, 256, 2 * GUARD + offset + rows * stride).astype(np.uint8) if fill is None else \
        np.full(2 * GUARD + offset + rows * stride, fill, np.uint8)
    body = flat[GUARD + offset:GUARD + offset + rows * stride].reshape(rows, stride)
    body[:, :L] = a
    return flat, dev(flat)


def body(flat, rows, stride, offset=0):
    return flat[GUARD + offset:GUARD + offset + rows * stride].reshape(rows, stride)


def check(eng, n, L, plane_stride, ev_stride, assoc_stride, mode, offset=0, variant=0, seed=0, params=(HIT, MISS, CMAX), view_range=RANGE,
          ndet=K, label=""):
    """One launch against the spec.  mode: "dup" (out of place through repeated, out-of-order ancestors), "id" (out of place, the
    identity index), "none" (out of place, no index), "inplace".  -> the spec's stats and the device's evidence buffer."""
    rng = np.random.default_rng(seed + 1)
    rows = n + 3 if mode == "dup" else n
    anc = {"dup": rng.integers(0, rows, n).astype(np.int32), "id": np.arange(n, dtype=np.int32), "none": None, "inplace": None}[mode]
    x, y, mp, tab, c, ev = make_case(n, L, plane_stride, rows, variant, seed, params)
    src = np.arange(n) if anc is None else anc
    ev[src] = c                              # (duplicates: the last writer wins; the spec reads what the kernel reads)
    h_tab, d_tab = guarded(tab, assoc_stride, offset, seed=seed + 2)
    h_in, d_in = guarded(ev, ev_stride, offset, seed=seed + 3)
    ev_in = body(h_in, rows, ev_stride, offset)
    in_place = mode == "inplace"
    want_mp, want_ev, want_st = E.evidence(mp, x, y, anc, body(h_tab, n, assoc_stride, offset), ndet, ev_in, *params, view_range, L=L,
                                           in_place=in_place)
    if in_place:
        h_out, d_out = h_in, d_in
    else:
        h_out, d_out = guarded(np.zeros((n, 0), np.uint8), ev_stride, offset, fill=7)
    want_flat = h_out.copy()
    body(want_flat, n, ev_stride, offset)[:] = want_ev
    d_mp = dev(mp)
    d_st = torch.full((n, 2), -1, dtype=torch.int32, device=DEV)
    at = GUARD + offset
    eng.landmark_evidence_dev(d_mp, 5 * plane_stride, plane_stride, L, dev(x), dev(y), dev(anc) if anc is not None else None, n,
                              d_tab[at:], assoc_stride, d_in[at:], d_out[at:], ev_stride, *params, view_range, d_st)
    got_flat, got_mp, got_st = host(d_out), host(d_mp), host(d_st)
    assert np.array_equal(got_flat, want_flat), f"{label}: evidence differs at {np.argwhere(got_flat != want_flat)[:5].ravel().tolist()}"
    assert np.array_equal(bits(got_mp), bits(want_mp)), f"{label}: map rows"      # the whole buffer: padding and unpruned planes untouched
    assert np.array_equal(got_st, want_st), f"{label}: stats"
    assert np.array_equal(host(d_tab), h_tab), f"{label}: the table changed"
    if not in_place:
        assert np.array_equal(host(d_in), h_in), f"{label}: the source evidence changed"
    return want_st, got_flat, (mp, want_mp)


def configs(L):
    """(plane_stride, ev_stride, assoc_stride, mode, offset): plane_stride = L rounded up to 32 and larger; byte strides both
    multiples of 4 (the dword path) and not, and a base offset by one byte (the byte path)."""
    Lp, L4 = (L + 31) // 32 * 32, (L + 3) // 4 * 4
    odd = L + 1 if (L + 1) % 4 else L + 2
    return ((Lp, Lp, L4 + 4, "dup", 0), (Lp + 32, odd, L + 3 if (L + 3) % 4 else L + 5, "id", 0), (Lp, L4, Lp, "inplace", 0),
            (Lp + 64, odd, L4, "inplace", 0), (Lp, L4 + 8, L4, "dup", 1), (Lp, L4, L4, "none", 0), (Lp, L4, L4 + 4, "inplace", 1))


@pytest.mark.parametrize("L", LS)
@pytest.mark.parametrize("n", NS)
def test_evidence_equals_the_spec(eng, n, L):
    """Every configuration; the scenarios rotate through the landmarks, so every branch occurs in every launch once there are 16
    landmarks in it — smaller shapes run all 16 rotations."""
    for j, (ps, es, ts, mode, offset) in enumerate(configs(L)):
        pruned = seen = 0
        for variant in (range(len(SCENARIOS)) if n * L < len(SCENARIOS) else (j,)):
            st, _, (mp, want_mp) = check(eng, n, L, ps, es, ts, mode, offset, variant, seed=100 * n + L + j, label=f"n={n} L={L} config {j} v{variant}")
            pruned += int(st[:, 0].sum())
            seen += int(st[:, 1].sum())
        assert pruned > 0 and seen > 0   # (the cases exercise both outcomes)


def test_longest_row(eng):
    """L = SLAM_MAX_OBS with 3 particles: 64 batches, both paths."""
    L = 8192
    for j, (ps, es, ts, mode, offset) in enumerate(((L, L, L, "dup", 0), (L + 32, L + 1, L + 2, "dup", 0), (L, L, L, "inplace", 0))):
        st, _, _ = check(eng, 3, L, ps, es, ts, mode, offset, variant=j, seed=j, label=f"L=8192 config {j}")
        assert st[:, 0].sum() > 0


@pytest.mark.parametrize("params", [(255, 1, 255), (1, 255, 255), (255, 255, 1), (1, 1, 1), (7, 200, 100)])
def test_parameter_extremes(eng, params):
    """Any evidence byte in 0 .. 255 under extreme parameters: c = 200, hit = 255 does not wrap; an evidence above cmax comes down."""
    for mode, es in (("dup", 132), ("inplace", 131)):
        check(eng, 65, 129, 160, es, es, mode, seed=sum(params), params=params, label=f"{params} {mode}")


def test_no_detections_and_all_of_them(eng):
    try:
        eng.detections_upload(np.zeros(0, F), np.zeros(0, F))
        st, _, _ = check(eng, 5, 65, 96, 68, 68, "dup", ndet=0, label="K = 0")   # an observing frame: every visible seen landmark takes a miss
        assert st[:, 0].sum() > 0
        eng.detections_upload(np.zeros(64, F), np.zeros(64, F))
        check(eng, 5, 65, 96, 68, 68, "dup", ndet=64, label="K = 64")
        check(eng, 5, 65, 96, 67, 67, "inplace", ndet=64, label="K = 64 in place")
    finally:
        eng.detections_upload(np.zeros(K, F), np.zeros(K, F))


def test_view_range_edges(eng):
    check(eng, 5, 65, 96, 68, 68, "dup", view_range=1e30, label="range2 = inf")   # every finite mean is visible
    check(eng, 5, 65, 96, 68, 68, "dup", view_range=1e-30, label="range2 = 0")
    check(eng, 5, 65, 96, 68, 68, "dup", view_range=0.1, label="range 0.1")


def test_two_runs_give_the_same_bytes(eng):
    a = check(eng, 257, 500, 512, 512, 512, "dup", seed=9, label="first run")[1]
    b = check(eng, 257, 500, 512, 512, 512, "dup", seed=9, label="second run")[1]
    assert np.array_equal(a, b)


@pytest.mark.parametrize("L", (1, 63, 64, 65, 129, 500))
def test_init_equals_the_spec(eng, L):
    for n in (1, 5, 257):
        Lp = (L + 31) // 32 * 32
        _, _, mp, _, _, _ = make_case(n, L, Lp + 32, n, 0, L + n)
        d_mp = dev(mp)
        for stride, offset, value in ((Lp, 0, 8), (L + 1 if (L + 1) % 4 else L + 2, 0, 255), ((L + 3) // 4 * 4 + 4, 1, 1), (Lp, 0, 0)):
            h, d = guarded(np.zeros((n, 0), np.uint8), stride, offset, fill=7)
            want = h.copy()
            body(want, n, stride, offset)[:] = E.evidence_init(mp, value, L=L, ev_stride=stride)
            eng.evidence_init_dev(d_mp, 5 * (Lp + 32), Lp + 32, L, n, d[GUARD + offset:], stride, value)
            assert np.array_equal(host(d), want), f"init n={n} L={L} stride={stride} offset={offset}"
        assert np.array_equal(bits(host(d_mp)), bits(mp))


def test_argument_checks_and_counters(eng):
    pkg = load_package()
    n, L, Lp = 3, 31, 32
    x, y, mp, tab, c, _ = make_case(n, L, Lp, n, 0, 3)
    d_mp, d_x, d_y = dev(mp), dev(x), dev(y)
    d_tab = torch.full((n, Lp), 255, dtype=torch.uint8, device=DEV)
    d_in = torch.full((n, Lp), 5, dtype=torch.uint8, device=DEV)
    d_out = torch.full((n, Lp), 7, dtype=torch.uint8, device=DEV)
    d_anc = dev(np.zeros(n, np.int32))
    ok = dict(mp=d_mp, ps=Lp, L=L, x=d_x, y=d_y, anc=None, tab=d_tab, ts=Lp, ein=d_in, eout=d_out, es=Lp, hit=1, miss=1, cmax=8, vr=5.0)

    def call(e, **change):
        a = dict(ok, **change)
        e.landmark_evidence_dev(a["mp"], 5 * a["ps"], a["ps"], a["L"], a["x"], a["y"], a["anc"], n, a["tab"], a["ts"], a["ein"], a["eout"],
                                a["es"], a["hit"], a["miss"], a["cmax"], a["vr"], None)

    fresh = pkg.Engine(0)
    with pytest.raises(pkg.SlamError) as err:                       # no detections handed over
        call(fresh)
    assert err.value.status == -4 and fresh.evidence_counts() == (0, 0)
    fresh.close()
    c0 = eng.evidence_counts()
    for change in (dict(hit=0), dict(hit=256), dict(hit=-1), dict(miss=0), dict(miss=256), dict(cmax=0), dict(cmax=256),
                   dict(vr=0.0), dict(vr=-1.0), dict(vr=float("nan")), dict(vr=float("inf")), dict(L=8193, ps=8200, ts=8200, es=8200),
                   dict(ts=L - 1), dict(es=L - 1), dict(ps=L - 1), dict(anc=d_anc, eout=d_in), dict(mp=None), dict(x=None), dict(y=None),
                   dict(tab=None), dict(ein=None), dict(eout=None)):
        with pytest.raises(pkg.SlamError) as err:
            call(eng, **change)
        assert err.value.status == -2, change
    for bad in (dict(value=-1), dict(value=256), dict(es=L - 1), dict(ps=L - 1), dict(mp=None), dict(ev=None)):
        a = dict(dict(mp=d_mp, ps=Lp, es=Lp, ev=d_out, value=8), **bad)
        with pytest.raises(pkg.SlamError) as err:
            eng.evidence_init_dev(a["mp"], 5 * a["ps"], a["ps"], L, n, a["ev"], a["es"], a["value"])
        assert err.value.status == -2, bad
    # nothing was launched
    assert eng.evidence_counts() == c0 and np.all(host(d_out) == 7) and np.all(host(d_in) == 5) and np.array_equal(bits(host(d_mp)), bits(mp))
    a0, f0, i0 = eng.assoc_counts(), eng.ekf_form_counts(), eng.ekf_inplace_form_counts()
    call(eng)                                                       # (no stats wanted)
    call(eng, anc=d_anc)
    eng.evidence_init_dev(d_mp, 5 * Lp, Lp, L, n, d_out, Lp, 8)
    eng.sync()
    assert eng.evidence_counts() == (c0[0] + 2, c0[1] + 1)
    assert eng.assoc_counts() == a0 and eng.ekf_form_counts() == f0 and eng.ekf_inplace_form_counts() == i0
