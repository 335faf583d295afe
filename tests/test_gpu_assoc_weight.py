"""slam_assoc_weight_dev (csrc/assoc_weight_kernels.hip) and the _missed forms of the three evidence stages against
tests/_assoc_weight_spec.py, bit for bit: the six operations whatever the population, the counts and the constants (0, -0.0, a
denormal, a sum that reaches -inf), on the engine's buffer and on a user's; the miss count of each of the four forms of the
evidence stage, with map, evidence and stats byte for byte those of the call without it; the argument checks launch nothing."""
import numpy as np
import pytest
import torch

import _assoc_weight_spec as W
import _evidence_spec as E
import _fov_spec as V
import _sight_spec as S
import test_gpu_fov as TV
from __graft_entry__ import load_package
from conftest import bits
from test_assoc_weight_spec_cpu import plain_miss_now

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
LMAX = 40
CONSTANTS = [(-4.0, -1.5, -0.75), (0.0, 0.0, 0.0), (-0.0, -0.0, -0.0), (-1e-45, -3e-39, -1e-40), (-3.0e38, -1.0, -0.5), (-0.25, -3.0e38, -3.0e38),
             (0.0, -0.0, -2.0)]
dev, host = TV.dev, TV.host


@pytest.fixture(scope="module")
def eng(orc):
    e = load_package().Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def counts(n, seed):
    """Every value 0 .. 64 in each column of the stats, 0 .. LMAX in missed, whatever n (n = 1: one draw per call)."""
    rng = np.random.default_rng(seed)
    stats = np.stack([rng.permutation(np.resize(np.arange(65), max(n, 65)))[:n] for _ in range(3)], 1).astype(np.int32)
    missed = rng.permutation(np.resize(np.arange(LMAX + 1), max(n, LMAX + 1)))[:n].astype(np.int32)
    ll = (rng.standard_normal(n) * 30).astype(F)
    ll[::7] = 0.0
    return stats, missed, ll


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_stage_equals_the_spec(eng, n):
    if n >= 65:
        s, m, _ = counts(n, n)
        assert all(set(s[:, c]) == set(range(65)) for c in range(3)) and set(m) == set(range(LMAX + 1))
    c0 = eng.assoc_weight_count()
    launches = 0
    for k, consts in enumerate(CONSTANTS):
        for with_missed in (True, False):
            for user in (True, False):
                stats, missed, ll = counts(n, 10 * n + k)
                want, want_t = W.add(ll, stats, missed if with_missed else None, *consts)
                d_ll, d_t = dev(ll), torch.full((n,), 7.0, device=DEV)
                if user:
                    eng.assoc_weight_dev(dev(stats), dev(missed) if with_missed else None, n, *consts, d_ll, d_t)
                    got = host(d_ll)
                else:   # the engine's buffer: what a landmark update of n particles left (here: of no landmarks, every ll 0)
                    z = torch.zeros(n, device=DEV)
                    eng.detections_upload(np.zeros(1, F), np.zeros(1, F))
                    d_map = torch.full((n, 5, 4), -1.0, device=DEV)
                    d_tab = torch.full((n, 4), 255, dtype=torch.uint8, device=DEV)
                    eng.ekf_update_assoc_dev(d_map, d_map.clone(), 20, 4, 1, z, z, z, None, n, 0.01, d_tab, 4, None)
                    # twice: onto the update's zeros, then onto what the first call left (a buffer that is not 0)
                    first = (-0.5, -0.25, 0.0)
                    eng.assoc_weight_dev(dev(stats), None, n, *first, None, None)
                    eng.assoc_weight_dev(dev(stats), dev(missed) if with_missed else None, n, *consts, None, d_t)
                    d_lw = torch.empty(n, device=DEV)
                    eng.logweight_ekf_dev(None, 0.0, n, d_lw, None)
                    base = W.add(np.zeros(n, F), stats, None, *first)[0]
                    got, want = host(d_lw), W.add(base, stats, missed if with_missed else None, *consts)[0]
                    launches += 1
                launches += 1
                label = f"n={n} {consts} missed={with_missed} user={user}"
                assert np.array_equal(bits(host(d_t)), bits(want_t)), label + ": terms"
                if user:
                    assert np.array_equal(bits(got), bits(want)), label + ": log-likelihood"
                else:   # the weights' launch without a score or a carry: logw = ll' - 0
                    assert np.array_equal(got, want) and (n == 1 or (base != 0).any()), label + ": engine buffer"
                if k == 4 and n >= 65:
                    assert np.isneginf(want_t).any() and not np.isnan(want).any()   # the sum reaches -inf
    assert eng.assoc_weight_count() == c0 + launches


def test_stage_argument_checks(eng):
    pkg = load_package()
    n = 5
    stats, missed, ll = counts(n, 1)
    d_s, d_m, d_ll = dev(stats), dev(missed), dev(ll)
    c0 = eng.assoc_weight_count()
    for bad in (1e-30, 1.0, float("nan"), float("inf"), float("-inf")):
        for slot in range(3):
            c = [-1.0, -1.0, -1.0]
            c[slot] = bad
            with pytest.raises(pkg.SlamError) as err:
                eng.assoc_weight_dev(d_s, d_m, n, *c, d_ll)
            assert err.value.status == -2, (bad, slot)
    for call in (lambda: eng.assoc_weight_dev(None, d_m, n, -1.0, -1.0, -1.0, d_ll), lambda: eng.assoc_weight_dev(d_s, d_m, -1, -1.0, -1.0, -1.0, d_ll)):
        with pytest.raises(pkg.SlamError) as err:
            call()
        assert err.value.status == -2
    fresh = pkg.Engine(0)
    with pytest.raises(pkg.SlamError) as err:                       # no landmark update on this engine: no buffer to add to
        fresh.assoc_weight_dev(d_s, d_m, n, -1.0, -1.0, -1.0, None)
    assert err.value.status == -4 and fresh.assoc_weight_count() == 0
    fresh.assoc_weight_dev(d_s, d_m, 0, -1.0, -1.0, -1.0, None)     # ... but no particles need none
    assert fresh.assoc_weight_count() == 0
    fresh.close()
    assert eng.assoc_weight_count() == c0 and np.array_equal(bits(host(d_ll)), bits(ll))
    eng.assoc_weight_dev(d_s, d_m, 0, -1.0, -1.0, -1.0, d_ll)       # n = 0: nothing to do, nothing launched
    assert eng.assoc_weight_count() == c0


# ------------------------------------------------------------------ the evidence stages with the miss count
N = 300
HIT, MISS, CMAX, RANGE, MARGIN = TV.HIT, TV.MISS, TV.CMAX, TV.RANGE, TV.MARGIN
FORMS = ("plain", "sight", "fov", "fov+sight")


@pytest.mark.parametrize("K", [0, 1, 64])
@pytest.mark.parametrize("L", [1, 40, 65])
def test_evidence_counts_its_misses(eng, L, K):
    plane_stride, L4 = (L + 31) // 32 * 32 + 32, (L + 3) // 4 * 4
    zero = np.zeros(K, F)
    eng.detections_upload(zero, zero)
    seen_any = {f: 0 for f in FORMS}
    odd = L + 3 if (L + 3) % 2 else L + 4
    # the dword path and the byte path, each behind ancestors and in place
    for j, (ev_stride, assoc_stride, mode) in enumerate(((L4 + 4, L4 + 8, "behind"), (odd, L + 1, "inplace"), (L4 + 8, L4 + 4, "inplace"),
                                                         (odd, L + 2, "behind"))):
        rows = N + 3 if mode == "behind" else N
        rng = np.random.default_rng(1000 * L + 10 * K + j)
        anc = rng.permutation(rows)[:N].astype(np.int32) if mode == "behind" else None   # (a row per particle: the bytes of its own landmarks)
        (x, y, th), (bx, by), mp, tab, c, ev, _ = TV.make_case(N, L, plane_stride, rows, "sensor", seed=77 * L + K + j, k_dets=K)
        lo, hi = TV.ARCS["sensor"][0]
        src = np.arange(N) if anc is None else anc
        for i in range(N):
            ev[src[i]] = c[i]
        h_in = rng.integers(0, 256, (rows, ev_stride)).astype(np.uint8)
        h_in[:, :L] = ev
        h_tab = rng.integers(0, 256, (N, assoc_stride)).astype(np.uint8)
        h_tab[:, :L] = tab
        eng.scan_upload(bx, by)
        eng.sight_table_dev(128)
        T = S.table(bx, by, 128)
        in_place = mode == "inplace"
        plain = plain_miss_now(mp[:, :, :L], x, y, h_tab, K, RANGE)
        for form in FORMS:
            if form == "plain":
                w_mp, w_ev, w_st = E.evidence(mp, x, y, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, L=L, in_place=in_place)
                less = 0
            elif form == "sight":
                w_mp, w_ev, w_st, sp = S.evidence(mp, x, y, th, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, T, MARGIN, L=L, in_place=in_place)
                less = sp
            else:
                sight = form == "fov+sight"
                w_mp, w_ev, w_st, sp, ou = V.evidence(mp, x, y, th, anc, h_tab, K, h_in, HIT, MISS, CMAX, RANGE, lo, hi, T if sight else None,
                                                      MARGIN if sight else None, L=L, in_place=in_place)
                less = sp + ou
            want = W.missed_of(h_in, anc, w_ev, mp, w_mp, L)
            assert np.array_equal(want, plain - less), f"{form}: the spec's count is not the predicate's"
            outs = []
            for with_missed in (False, True):
                d_mp, d_in, d_tab = dev(mp), dev(h_in), dev(h_tab)
                d_out = d_in if in_place else torch.full((N, ev_stride), 7, dtype=torch.uint8, device=DEV)
                d_st = torch.full((N, 2), -1, dtype=torch.int32, device=DEV)
                d_sp, d_ou, d_ms = (torch.full((N,), -1, dtype=torch.int32, device=DEV) for _ in range(3))
                head = (d_mp, 5 * plane_stride, plane_stride, L, dev(x), dev(y))
                mid = (dev(anc) if anc is not None else None, N, d_tab, assoc_stride, d_in, d_out, ev_stride, HIT, MISS, CMAX, RANGE)
                ms = dict(d_missed=d_ms) if with_missed else {}
                if form == "plain":
                    eng.landmark_evidence_dev(*head, *mid, d_st, **ms)
                elif form == "sight":
                    eng.landmark_evidence_sight_dev(*head, dev(th), *mid, MARGIN, d_st, d_sp, **ms)
                else:
                    eng.landmark_evidence_fov_dev(*head, dev(th), *mid, MARGIN, float(lo), float(hi), form == "fov+sight", d_st, d_sp, d_ou, **ms)
                outs.append(tuple(host(t) for t in (d_mp, d_out, d_st, d_sp, d_ou, d_ms)))
            without, with_ = outs
            label = f"L={L} K={K} {mode} {form}"
            assert np.all(without[5] == -1) and np.array_equal(with_[5], want), f"{label}: missed {with_[5][:8].tolist()} != {want[:8].tolist()}"
            for a, b, what in zip(without[:5], with_[:5], ("map rows", "evidence", "stats", "spared", "outside")):
                assert a.tobytes() == b.tobytes(), f"{label}: {what} differ from the call without the miss count"
            assert np.array_equal(with_[2], w_st) and np.array_equal(with_[1][:, :L], w_ev[:, :L]), f"{label}: not the spec's"
            seen_any[form] += int(want.sum())
    assert all(v > 0 for v in seen_any.values()), seen_any
