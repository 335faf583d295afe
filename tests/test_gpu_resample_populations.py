"""Every form of the resample tail on structured weight populations, against the exact integer restatement of
tests/_resample_exact.py: a single carrier on index 0, n - 1 and both sides of tile and block edges, whole zero tiles (equal
consecutive tile offsets in the tile-level search, equal pivots in the block-level one), workgroups whose slots span more than
two tiles (the un-staged branch of ancestors_from_scan_kernel<1>), shards without weight, the ESS gate on one carrier and on
equal weights, NaN log-weights, and the zero-total branch with its pinned values.

Forms: staged (prefix_sum / offspring_offsets / ancestors), fused (quantise_scan / offspring_from_scan / ancestors; single-GPU
and middle-shard), one launch (ancestors_from_scan: kPer = 1 up to 256 tiles, kPer = 16 above), sharded (offspring_from_scan_
sharded / ancestors_sharded / migrate_pack), gated (one launch, and fused through the sharded entry with one and three ranks)
and the C session (rows, split with and without survivor rows) from a kidnapped start and across a frame of total weight 0.
"""
import numpy as np
import pytest
import torch

import _resample_exact as X
from __graft_entry__ import load_package
from conftest import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, FRAME = 0x1234567887654321, 5
SIZES = [1, 2, 33, 2047, 2048, 2049, 3 * 2048 + 5, 6 * 2048]
BIG1 = 256 * 2048              # the largest shape of ancestors_from_scan_kernel<1>
BIG16 = 257 * 2048 + 7         # the smallest of ancestors_from_scan_kernel<16>
BIG16_NAMES = ["carrier@0", f"carrier@{BIG16 - 1}", "one_per_tile", f"carrier@{256 * 2048 + 3}", "leading_zero_tiles",
               "all_equal", "sparse_tiles"]


@pytest.fixture(scope="module")
def eng():
    pkg = load_package()
    e = pkg.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


@pytest.fixture(scope="module")
def gated():
    """an engine of its own for the gate: the carried weights and the flag live in the engine"""
    pkg = load_package()
    e = pkg.Engine(0)
    e.set_stream(torch.cuda.current_stream().cuda_stream)
    yield e
    torch.cuda.synchronize()
    e.close()


def dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _i64(v):
    return dev(np.array([v], np.uint64).view(np.int64))


def _f32(v):
    return dev(np.array([v], np.float32))


def _cases(sizes):
    return [(n, name) for n in sizes for name in X.names(n)]


def _entry(n, name):
    e = X.population(n, name)
    return e["logw"], e.get("max")


# ------------------------------------------------------------------ the forms, each returning host arrays


def _load(eng, logw, m, want_max):
    """log-weights into the engine as the weights' launch leaves them (score = None, gain 0: logw = loglik exactly)
    -> (d_logw, d_max or None).  m: an outside maximum to quantise against (then always handed over as d_max)."""
    n = len(logw)
    d_logw = torch.empty(n, device=DEV)
    d_max = torch.empty(1, device=DEV) if (want_max or m is not None) else None
    eng.logweight_dev(None, dev(logw), 0.0, n, d_logw, d_max)
    if m is not None:
        d_max = _f32(m)
    return d_logw, d_max


def staged(eng, logw, m=None):
    n = len(logw)
    d_logw, d_max = _load(eng, logw, m, True)
    wq, d_sum = torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(1, dtype=torch.int64, device=DEV)
    eng.quantise_weights_dev(d_logw, d_max, n, wq, d_sum)
    cdf = torch.empty(n, dtype=torch.int64, device=DEV)
    eng.prefix_sum_dev(wq, n, cdf)
    first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.offspring_offsets_dev(cdf, n, None, d_sum, SEED, FRAME, n, first)
    anc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.ancestors_dev(first, n, 0, n, anc)
    return host(wq).view(np.uint64), int(host(d_sum).view(np.uint64)[0]), host(first), host(anc)


def fused(eng, logw, m=None):
    n = len(logw)
    d_logw, d_max = _load(eng, logw, m, False)
    eng.quantise_scan_dev(d_logw, d_max, n, None)
    first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.offspring_from_scan_dev(n, None, None, SEED, FRAME, n, first)
    anc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.ancestors_dev(first, n, 0, n, anc)
    return host(first), host(anc)


def fused_middle_shard(eng, logw, m, base, total, n_total):
    n = len(logw)
    d_logw, d_max = _load(eng, logw, m, True)
    d_sum = torch.full((1,), -1, dtype=torch.int64, device=DEV)
    eng.quantise_scan_dev(d_logw, d_max, n, d_sum)
    first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.offspring_from_scan_dev(n, _i64(base), _i64(total), SEED, FRAME, n_total, first)
    return int(host(d_sum).view(np.uint64)[0]), host(first)


def one_launch(eng, logw, m=None):
    n = len(logw)
    d_logw, d_max = _load(eng, logw, m, False)
    eng.quantise_scan_dev(d_logw, d_max, n, None)
    anc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    eng.ancestors_from_scan_dev(n, SEED, FRAME, anc)
    return host(anc)


# ------------------------------------------------------------------ the catalogue through every unsharded form


@pytest.mark.parametrize("n,name", _cases(SIZES))
def test_staged_and_fused_forms(eng, n, name):
    logw, m = _entry(n, name)
    wq, total, anc, first = X.reference(n, name, SEED, FRAME)
    g_wq, g_total, g_first, g_anc = staged(eng, logw, m)
    assert np.array_equal(g_wq, wq) and g_total == total
    assert np.array_equal(g_first, first), "staged first"
    assert np.array_equal(g_anc, anc), "staged ancestors"
    g_first, g_anc = fused(eng, logw, m)
    assert np.array_equal(g_first, first), "fused first"
    assert np.array_equal(g_anc, anc), "fused ancestors"
    # the same tile as the middle shard of three: twice its weight in front of it, four times in all
    base, tot3, n3 = 2 * total, 4 * total, 3 * n
    _, want = X.exact_ancestors(wq, SEED, FRAME, n_total=n3, base=base, total=tot3)
    g_total, g_first = fused_middle_shard(eng, logw, m, base, tot3, n3)
    assert g_total == total and np.array_equal(g_first, want), "fused first as a middle shard"
    if X.population(n, name).get("identity"):
        assert np.array_equal(g_anc, np.arange(n))


@pytest.mark.parametrize("n,name", _cases(SIZES + [BIG1]) + [(BIG16, name) for name in BIG16_NAMES])
def test_one_launch_form(eng, n, name):
    logw, m = _entry(n, name)
    wq, total, anc, first = X.reference(n, name, SEED, FRAME)
    if name == "sparse_tiles":   # the un-staged branch is really taken: some workgroup's slots span more than two tiles
        assert X.broken_promises({"wg_span": 4}, wq, anc) == []
    got = one_launch(eng, logw, m)
    assert got.min() >= 0 and got.max() < n
    bad = np.flatnonzero(got != anc)
    assert bad.size == 0, f"{bad.size} slots differ, the first: slot {bad[0]} got {got[bad[0]]} want {anc[bad[0]]}"
    if X.population(n, name).get("identity"):
        assert np.array_equal(got, np.arange(n))


# ------------------------------------------------------------------ NaN among finite log-weights


@pytest.mark.parametrize("n", [7, 2049, 4097])
def test_nan_log_weight_is_weight_zero_in_every_form(eng, n):
    for name, logw in X.nan_cases(n).items():
        wq, total = X.quantised(logw)
        anc, first = X.exact_ancestors(wq, SEED, FRAME)
        g_wq, g_total, g_first, g_anc = staged(eng, logw)
        assert np.array_equal(g_wq, wq) and g_total == total and np.array_equal(g_first, first) and np.array_equal(g_anc, anc), name
        g_first, g_anc = fused(eng, logw)
        assert np.array_equal(g_first, first) and np.array_equal(g_anc, anc), name
        assert np.array_equal(one_launch(eng, logw), anc), name


# ------------------------------------------------------------------ sharded: plan, pack and ancestors


def _sharded(eng, logw, m, world):
    """`world` equal shards of one population, one after the other on this engine -> (first_all, per rank: global ancestors,
    src, plan) with the packed rows compared against the numpy restatement on the way."""
    from _oracle_ops import OracleOps
    from _pf_rehearsal import HipOps

    n_total = len(logw)
    n = n_total // world
    assert n * world == n_total
    lw, own = X.oracle.logweight(None, logw, 0.0)
    d_max = _f32(own if m is None else m)
    totals = torch.zeros(world, dtype=torch.int64, device=DEV)
    first_all = torch.full((n_total,), -7, dtype=torch.int32, device=DEV)
    for rnd in range(2):   # the shards' totals first (what the ranks all-gather), then every rank's offsets
        for r in range(world):
            eng.quantise_scan_dev(dev(logw[r * n:(r + 1) * n]), d_max, n, totals[r:r + 1])
            if rnd:
                eng.offspring_from_scan_sharded_dev(n, totals, r, world, SEED, FRAME, n_total, first_all[r * n:(r + 1) * n])
    cpu, gpu = OracleOps(None, None, None, None), HipOps(eng)
    rng = np.random.default_rng(n_total)
    L, Lp, cap = 3, 4, 2 * n
    pose = rng.standard_normal((3, cap)).astype(np.float32)
    mp = rng.standard_normal((cap, 5, Lp)).astype(np.float32)
    h_first = host(first_all)
    out = []
    for r in range(world):
        src_c, plan_c = torch.zeros(n, dtype=torch.int32), torch.zeros(1 + 3 * world, dtype=torch.int32)
        cpu.ancestors_sharded(torch.from_numpy(h_first), n_total, n, r, world, src_c, plan_c)
        src_g = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        plan_g = torch.zeros(1 + 3 * world, dtype=torch.int32, device=DEV)
        pidx = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        gpu.ancestors_sharded(first_all, n_total, n, r, world, src_g, plan_g, pidx)
        assert np.array_equal(host(plan_g), plan_c.numpy()), f"rank {r}: plan"
        assert gpu.read_plan(plan_g, world) == plan_c.tolist()
        assert np.array_equal(host(src_g), src_c.numpy()), f"rank {r}: gather index"
        plan = plan_c.tolist()
        stot, rec = sum(plan[1:1 + world]), 3 + 5 * L
        out_c, out_g = torch.zeros(rec * stot), torch.zeros(rec * stot, device=DEV)
        cpu.migrate_pack(n, r, world, plan, torch.from_numpy(pose), cap, torch.from_numpy(mp), 5 * Lp, Lp, L, out_c)
        gpu.migrate_pack(n, r, world, plan, dev(pose), cap, dev(mp), 5 * Lp, Lp, L, out_g)
        assert np.array_equal(bits(host(out_g)), bits(out_c.numpy())), f"rank {r}: packed rows"
        p = host(pidx).astype(np.int64)   # owner * 3n + local index: the global ancestor of every slot of this rank
        out.append(dict(anc=(p // (3 * n)) * n + p % (3 * n), src=host(src_g), plan=plan))
    return h_first, host(totals).view(np.uint64), out


@pytest.mark.parametrize("n_total,world,name", [
    (6 * 2048, 3, "carrier@2048"), (6 * 2048, 3, "leading_zero_tiles"), (6 * 2048, 3, "sparse_tiles"),
    (6 * 2048, 3, "trailing_zero_tiles"), (6 * 2048, 4, "carrier@0"), (6 * 2048, 4, "carrier@12287"),
    (6 * 2048, 4, "carrier@10240"), (6 * 2048, 4, "leading_zero_tiles"), (6 * 2048, 4, "one_per_tile"),
    (6 * 2048, 4, "tiny_and_sparse"), (6 * 2048, 4, "equal_run_over_tile_edge"),
    (3 * 2049, 3, "carrier@0"), (3 * 2049, 3, "carrier@6146"), (3 * 2049, 3, "leading_zero_tiles"),
    (3 * 2049, 3, "one_per_tile"), (3 * 2049, 3, "all_equal")])
def test_sharded_form(eng, n_total, world, name):
    logw, m = _entry(n_total, name)
    wq, total, anc, first = X.reference(n_total, name, SEED, FRAME)
    n = n_total // world
    share = [int(np.sum(wq[r * n:(r + 1) * n].astype(object))) for r in range(world)]
    g_first, g_totals, ranks = _sharded(eng, logw, m, world)
    assert g_totals.tolist() == share
    assert np.array_equal(g_first, first)
    for r, res in enumerate(ranks):
        assert np.array_equal(res["anc"], anc[r * n:(r + 1) * n]), f"rank {r}: ancestors"
        plan = res["plan"]
        if share[r] == 0:   # a shard without weight sends nothing and receives every one of its rows
            assert sum(plan[1:1 + world]) == 0 and (res["src"] >= n).all()
            assert sum(plan[1 + world:1 + 2 * world]) == len(np.unique(anc[r * n:(r + 1) * n]))
    if name.startswith("carrier@"):   # the shard with the only carrier sends that one row to every other rank
        owner = int(name[8:]) // n
        assert share[owner] == total
        for r, res in enumerate(ranks):
            want = [0] * world
            if r != owner:
                want[owner] = 1
            assert res["plan"][1 + world:1 + 2 * world] == want
            assert res["plan"][1:1 + world] == ([1 if q != owner else 0 for q in range(world)] if r == owner else [0] * world)
    if name == "leading_zero_tiles":
        assert share[0] == 0


# ------------------------------------------------------------------ gated


def _gated_frame(e, frac, logw, form):
    """one gated resample stage on a fresh gate -> (ancestors, host flag, the log-weights of a probe frame behind it, which
    shows both the device flag and the carry: carry + probe where the flag says `kept`, the probe alone where not)"""
    n = len(logw)
    e.resample_gate_set(frac)
    d_logw = torch.empty(n, device=DEV)
    e.logweight_dev(None, dev(logw), 0.0, n, d_logw, None)
    anc = torch.full((n,), -7, dtype=torch.int32, device=DEV)
    sums = None
    if form == "one_launch":
        e.quantise_scan_dev(d_logw, None, n, None)
        e.ancestors_from_scan_dev(n, SEED, FRAME, anc)
    else:   # fused: the sharded entry with one rank, fed by the (total, S, Q) triple of the scan
        d_sums = torch.full((3,), -1, dtype=torch.int64, device=DEV)
        e.quantise_scan_dev(d_logw, None, n, d_sums)
        first = torch.full((n,), -7, dtype=torch.int32, device=DEV)
        e.offspring_from_scan_sharded_dev(n, d_sums, 0, 1, SEED, FRAME, n, first)
        e.ancestors_dev(first, n, 0, n, anc)
        sums = [int(v) for v in host(d_sums).view(np.uint64)]
    flag = e.resample_happened()
    probe = (np.arange(n) % 5).astype(np.float32) * np.float32(0.25) - np.float32(1.0)
    nxt = torch.empty(n, device=DEV)
    e.logweight_dev(None, dev(probe), 0.0, n, nxt, None)
    return host(anc), flag, probe, host(nxt), sums


def _check_gated(orc, e, frac, logw, form, must=None):
    n = len(logw)
    lw, m = orc.logweight(None, logw, 0.0)
    wq, total = orc.quantise_weights(lw, m)
    s16, q16 = orc.ess_terms(wq)
    fq = orc.ess_frac_q16(frac)
    assert fq != 0
    resample = orc.ess_resample(s16, q16, n, fq)
    if must is not None:
        assert resample == must
    anc, flag, probe, nxt, sums = _gated_frame(e, frac, logw, form)
    want = X.exact_ancestors(wq, SEED, FRAME)[0] if resample else np.arange(n)
    assert flag == resample, "verdict"
    assert np.array_equal(anc, want), "ancestors"
    if sums is not None:
        assert sums == [total, s16, q16]
    carry = None if resample else orc.weight_carry(lw, m)
    want_nxt = orc.logweight_carry(None, probe, 0.0, carry)[0]
    if np.isnan(want_nxt).any():   # (inf - inf: the sign of a NaN is not part of the contract)
        assert np.array_equal(np.isnan(nxt), np.isnan(want_nxt))
        ok = ~np.isnan(want_nxt)
        assert np.array_equal(bits(nxt[ok]), bits(want_nxt[ok])), "device flag / carry"
    else:
        assert np.array_equal(bits(nxt), bits(want_nxt)), "device flag / carry"
    return resample


@pytest.mark.parametrize("form", ["one_launch", "fused"])
@pytest.mark.parametrize("frac", [0.05, 0.5, 0.9])
@pytest.mark.parametrize("n", [2049, 6 * 2048])
def test_gated_forms(orc, gated, n, frac, form):
    pops = X.populations(n)
    for name in ("carrier@0", f"carrier@{n - 1}", "carrier@2048"):       # ESS = 1: resamples at every threshold
        assert _check_gated(orc, gated, frac, pops[name]["logw"], form, must=True), name
    assert not _check_gated(orc, gated, frac, pops["all_equal"]["logw"], form, must=False)   # ESS = n: keeps its population
    _check_gated(orc, gated, frac, pops["leading_zero_tiles"]["logw"], form)   # in between: the specification's verdict
    _check_gated(orc, gated, frac, pops["equal_run_over_tile_edge"]["logw"], form)


def test_gated_in_between_entry_goes_both_ways(orc):
    n = 6 * 2048
    wq, _ = X.quantised(X.populations(n)["leading_zero_tiles"]["logw"])
    s16, q16 = orc.ess_terms(wq)
    assert [orc.ess_resample(s16, q16, n, orc.ess_frac_q16(f)) for f in (0.05, 0.5, 0.9)] == [False, False, True]


# ------------------------------------------------------------------ the zero-total branch: pinned values


@pytest.mark.parametrize("n", [7, 2049, 4097])
def test_zero_total_pinned_values(orc, eng, gated, n):
    last = np.full(n, n - 1)
    for name, logw in X.zero_total_cases(n).items():
        g_wq, g_total, g_first, g_anc = staged(eng, logw)
        assert not g_wq.any() and g_total == 0 and not g_first.any() and np.array_equal(g_anc, last), f"staged, {name}"
        g_first, g_anc = fused(eng, logw)
        assert not g_first.any() and np.array_equal(g_anc, last), f"fused, {name}"
        g_total, g_first = fused_middle_shard(eng, logw, None, 0, 0, 3 * n)
        assert g_total == 0 and not g_first.any(), f"fused as a shard, {name}"
        assert np.array_equal(one_launch(eng, logw), last), f"one launch, {name}"
        for form in ("one_launch", "fused"):   # under a gate: S = Q = 0 keeps the population, carry = logw - max as computed
            assert not _check_gated(orc, gated, 0.5, logw, form, must=False), f"gated {form}, {name}"


@pytest.mark.parametrize("n_total,world", [(3 * 7, 3), (3 * 2049, 3), (3 * 4097, 3), (4 * 1025, 4)])
def test_zero_total_sharded(eng, n_total, world):
    """every rank sees first = 0 everywhere: every slot descends from the last particle of the last rank, which sends that one
    row once to each of the others"""
    n = n_total // world
    for name, logw in X.zero_total_cases(n_total).items():
        g_first, g_totals, ranks = _sharded(eng, logw, None, world)
        assert not g_totals.any() and not g_first.any(), name
        for r, res in enumerate(ranks):
            assert (res["anc"] == n_total - 1).all(), name
            sent, received = res["plan"][1:1 + world], res["plan"][1 + world:1 + 2 * world]
            if r == world - 1:
                assert (res["src"] == n - 1).all() and sent == [1] * (world - 1) + [0] and received == [0] * world, name
            else:
                assert (res["src"] == n).all() and sent == [0] * world and received == [0] * (world - 1) + [1], name


@pytest.mark.parametrize("frac", [0.05, 0.5, 0.9])
@pytest.mark.parametrize("n", [7, 4097])
def test_zero_total_gated_on_three_ranks(gated, n, frac):
    """S = Q = 0 summed over the ranks: no resample, every rank writes the identity first = rank * n + i, flag 0"""
    world = 3
    for name, logw in X.zero_total_cases(world * n).items():
        gated.resample_gate_set(frac)
        _, own = X.oracle.logweight(None, logw, 0.0)
        d_max = _f32(own)
        sums = torch.full((3 * world,), -1, dtype=torch.int64, device=DEV)
        first_all = torch.full((world * n,), -7, dtype=torch.int32, device=DEV)
        for rnd in range(2):
            for r in range(world):
                gated.quantise_scan_dev(dev(logw[r * n:(r + 1) * n]), d_max, n, sums[3 * r:3 * r + 3])
                if rnd:
                    gated.offspring_from_scan_sharded_dev(n, sums, r, world, SEED, FRAME, world * n, first_all[r * n:(r + 1) * n])
                    assert not gated.resample_happened(), name
        assert not host(sums).any(), name
        assert np.array_equal(host(first_all), np.arange(world * n)), name


# ------------------------------------------------------------------ the C session


def _session_world():
    import test_gpu_survivor_rows as S

    return S, S._world()


def _open(n, layout, on, poses):
    S, w = _session_world()
    B, pkg = w["B"], load_package()
    e = pkg.Engine(0)
    e.survivor_rows_set(on)
    e.profile_enable(e.PROF_MATERIALISE)
    e.grid_set_dev(0, w["d_edt"], pkg.grid_meta(S.GRID, S.GRID, S.GRID, *w["meta"]))
    ses = pkg.PfSession(e, n, S.L, sigma=B.SIGMA, meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN, seed=S.SEED, map_layout=layout)
    ses.set_poses(*poses)
    ses.set_map_dev(w["m0"][:n], 5 * S.LP, S.LP)
    e.sync()
    return e, ses


def _spec_loop(n, poses):
    """the frame loop of tests/_pf_rehearsal.py on the CPU specification's stages (the EDT is the session's own)"""
    from _oracle_ops import OracleOps
    from _pf_rehearsal import ParticleFilter

    S, w = _session_world()
    B = w["B"]
    meta = X.oracle.meta(S.GRID, S.GRID, S.GRID, *w["meta"])
    cpu = ParticleFilter(OracleOps(meta, w["d_edt"].cpu().numpy(), None, None), n, S.L, device="cpu", seed=S.SEED, sigma=B.SIGMA,
                         meas_var=B.MEAS_VAR, score_gain=B.SCORE_GAIN)
    cpu.set_poses(*poses)
    cpu.set_map(w["m0_host"][:n, :, :S.L])
    return cpu


def _frame(sessions, cpu, fr, n, launches, equal_nan=False):
    """one frame on every session and on the specification loop -> the specification's (log-weights, ancestors); the
    sessions' poses, log-weights, ancestors and the map rows of every slot (read through the pending gather: with survivor
    rows on only the rows of marked particles exist, and no settle may run for the read) are its bits"""
    S, w = _session_world()
    cpu.ops.bx, cpu.ops.by = fr["bx"], fr["by"]
    cpu.step(fr["dp"], (fr["ids"], fr["zx"], fr["zy"]))
    want = dict(pose=cpu.pose[cpu.cur].numpy(), logw=cpu.logw.numpy(), anc=cpu.src_idx.numpy(), rows=cpu.maps().numpy())
    for what, (e, ses) in sessions.items():
        S._step(e, ses, fr)
        launches[what] = launches.get(what, 0) + e.profile_read(e.PROF_MATERIALISE)[1]   # (reading the bracket clears it)
        rows = ses.map_rows(np.arange(n, dtype=np.int32))
        assert e.profile_read(e.PROF_MATERIALISE)[1] == 0, f"{what}: reading rows through the gather settled"
        e.sync()
        v = ses.device_view()
        got = dict(rows=rows, **{k: S._tensor(v[k]).cpu().numpy() for k in ("pose", "logw", "anc")})
        for k in want:
            if equal_nan and got[k].dtype == np.float32:   # (the sign of a NaN born on the CPU is not the device's)
                assert np.array_equal(got[k], want[k], equal_nan=True), f"{what}: {k}"
            else:
                assert np.array_equal(got[k].view(np.uint32), np.ascontiguousarray(want[k]).view(np.uint32)), f"{what}: {k}"
    return want["logw"], want["anc"]


def _close(sessions):
    for e, ses in sessions.values():
        ses.close()
        e.close()


@pytest.mark.parametrize("n,carrier", [(n, c) for n in (2049, 4097) for c in dict.fromkeys((0, 2048, n - 1))])
def test_sessions_from_a_kidnapped_start(n, carrier):
    """Frame 0 of a kidnapped start: every pose but one far from the truth, so that one particle carries all the weight; three
    frames of a rows session and of a split session with survivor rows on and off (n = 4097: frames 1 and 2 run the
    fused front launch, the ancestor search marks the survivors and only their rows are written) against the
    specification loop, bit for bit, and the ancestors of every frame against the exact integers."""
    S, w = _session_world()
    p0 = w["B"].true_pose(0)
    poses = [np.full(n, np.float32(p0[k]) + np.float32(d), np.float32) for k, d in enumerate((3.0, -2.0, 1.0))]
    for k in range(3):
        poses[k][carrier] = np.float32(p0[k])
    sessions = {"rows": _open(n, "rows", True, poses), "split, survivor rows": _open(n, "split", True, poses),
                "split, every row": _open(n, "split", False, poses)}
    cpu = _spec_loop(n, poses)
    launches = {}
    for f in range(3):
        logw, anc = _frame(sessions, cpu, w["fr"][f], n, launches)
        wq, total = X.quantised(logw)
        if f == 0:   # what the start promises
            assert np.flatnonzero(wq).tolist() == [carrier] and (anc == carrier).all()
        assert np.array_equal(anc, X.exact_ancestors(wq, S.SEED, f)[0]), f"frame {f}"
    if n == 4097:   # the survivor frames really ran (frames 1 and 2: the launch behind the search, and a settle for the views)
        assert launches["split, survivor rows"] >= 2
    assert launches["split, every row"] == 0 and launches["rows"] == 0
    _close(sessions)


def test_sessions_across_a_frame_of_total_weight_zero():
    """Frame 1 observes every landmark at +inf: every log-likelihood is -inf or NaN, the grand total 0.  The pinned rule in the
    session: every slot descends from particle n - 1; with survivor rows on the search marks particle n - 1 and nobody else
    can be read, so the rows of all n slots, read without a settle, are that one row — the bits of the sessions that write
    every row; frame 2 gathers through those ancestors, and is such a frame again."""
    S, w = _session_world()
    n = 4097
    poses = [p[:n] for p in w["poses"]]
    sessions = {"rows": _open(n, "rows", True, poses), "split, survivor rows": _open(n, "split", True, poses),
                "split, every row": _open(n, "split", False, poses)}
    cpu = _spec_loop(n, poses)
    launches = {}
    for f in range(3):
        fr = w["fr"][f]
        if f == 1:
            fr = dict(fr, zx=np.full_like(fr["zx"], np.inf))
        logw, anc = _frame(sessions, cpu, fr, n, launches, equal_nan=f >= 1)
        wq, total = X.quantised(logw)
        assert (total == 0) == (f >= 1)   # (frame 2 starts from the one row frame 1 left: means at infinity, total 0 again)
        if f >= 1:
            assert not np.isfinite(logw).any() and (anc == n - 1).all()
        assert np.array_equal(anc, X.exact_ancestors(wq, S.SEED, f)[0]), f"frame {f}"
    assert launches["split, survivor rows"] >= 2 and launches["split, every row"] == 0
    _close(sessions)
