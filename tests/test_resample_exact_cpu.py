"""The CPU specification of the resample (oracle.resample / offspring_offsets / ancestors) against the exact restatement in
Python integers (tests/_resample_exact.py) on the catalogue of structured populations; the properties that need no
reference; the promises of the catalogue; the zero-total rule of DESIGN.md section 7.  No GPU."""
import numpy as np
import pytest

import _resample_exact as X

SEED, FRAME = 0x1234567887654321, 5
SIZES = [1, 2, 33, 2047, 2048, 2049, 3 * 2048 + 5, 6 * 2048]


def _cases():
    return [(n, name) for n in SIZES for name in X.populations(n)]


@pytest.mark.parametrize("n,name", _cases())
def test_specification_equals_exact_integers(orc, n, name):
    wq, total, anc, first = X.reference(n, name, SEED, FRAME)
    assert total == int(np.sum(wq.astype(object))) > 0
    assert orc.comb_offset(SEED, FRAME, total) == X.comb_offset(SEED, FRAME, total)
    got_first = orc.offspring_offsets(orc.prefix_sum(wq), 0, total, orc.comb_offset(SEED, FRAME, total), n)
    assert np.array_equal(got_first, first)
    assert np.array_equal(orc.ancestors(got_first, 0, n), anc)
    assert np.array_equal(orc.resample(wq, SEED, FRAME), anc)
    # what needs no reference
    assert (np.diff(anc) >= 0).all() and anc[0] >= 0 and anc[-1] < n
    assert (wq[anc] > 0).all()
    count = np.bincount(anc, minlength=n)
    w = [int(v) for v in wq]
    assert all(abs(int(c) * total - n * v) < total for c, v in zip(count, w))   # |count_i - n w_i / S| < 1, in integers


@pytest.mark.parametrize("n,name", _cases())
def test_catalogue_keeps_its_promises(n, name):
    wq, total, anc, first = X.reference(n, name, SEED, FRAME)
    assert X.broken_promises(X.populations(n)[name], wq, anc) == []


def test_required_entries_exist_where_the_sizes_allow():
    names = set(X.populations(6 * 2048))
    assert {"carrier@0", "carrier@12287", "carrier@2047", "carrier@2048", "carrier@10239", "carrier@10240", "carrier@31",
            "carrier@32", "carrier@2079", "carrier@2080", "one_per_tile", "sparse_tiles", "leading_zero_tiles",
            "trailing_zero_tiles", "all_equal", "all_tiny", "tiny_and_sparse", "tiny_then_dominant",
            "equal_run_over_tile_edge"} <= names
    assert "carrier@%d" % (256 * 2048 + 3) in X.names(257 * 2048 + 7)
    assert X.populations(1).keys() == {"carrier@0", "all_equal", "all_tiny"}


@pytest.mark.parametrize("name", ["sparse_tiles", "leading_zero_tiles", "trailing_zero_tiles", "carrier@2048", "one_per_tile"])
def test_a_promise_breaks_when_its_zero_tiles_are_filled(name):
    """the promises are asserted, not assumed: the same entry with weight in its empty tiles fails them"""
    n = 6 * 2048
    entry = dict(X.populations(n)[name])
    lw = entry["logw"].copy()
    lw[lw == X.ZERO] = X.TINY
    entry["logw"] = lw
    wq, _ = X.quantised(lw)
    anc, _ = X.exact_ancestors(wq, SEED, FRAME)
    assert X.broken_promises(entry, wq, anc) != []


def _cuts(n, n_shards):
    """cuts on and beside tile edges (a shard may be one particle, or hold no weight at all)"""
    edges = sorted({c for c in (2047, 2048, 2049, 4096, 3 * 2048 - 1, 4 * 2048) if 0 < c < n})
    return [0] + edges[:n_shards - 1] + [n]


@pytest.mark.parametrize("n,name,shards", [(6 * 2048, "sparse_tiles", 4), (6 * 2048, "leading_zero_tiles", 3),
                                           (6 * 2048, "carrier@10240", 5), (6 * 2048, "carrier@2048", 4),
                                           (3 * 2048 + 5, "one_per_tile", 4), (3 * 2048 + 5, "trailing_zero_tiles", 4),
                                           (2049, "carrier@2048", 3), (2049, "tiny_then_dominant", 3),
                                           (6 * 2048, "equal_run_over_tile_edge", 5), (6 * 2048, "tiny_and_sparse", 4)])
def test_sharded_specification_equals_exact_integers(orc, n, name, shards):
    wq, total, anc, first = X.reference(n, name, SEED, FRAME)
    cuts = _cuts(n, shards)
    assert len(cuts) == shards + 1
    cdf = np.concatenate([[0], np.cumsum(wq.astype(object))])
    u = orc.comb_offset(SEED, FRAME, total)
    first_all, counts, empty = np.empty(n, np.int32), [], 0
    for a, b in zip(cuts[:-1], cuts[1:]):
        base = int(cdf[a])
        empty += int(cdf[b]) == base
        first_all[a:b] = orc.offspring_offsets(orc.prefix_sum(wq[a:b]), base, total, u, n)
        cnt, f = X.exact_ancestors(wq[a:b], SEED, FRAME, n_total=n, base=base, total=total)
        assert np.array_equal(first_all[a:b], f) and np.array_equal(f, first[a:b])
        counts.append(cnt)
    assert np.array_equal(X.join_shards(counts, n), anc)
    for a, b in zip(cuts[:-1], cuts[1:]):
        assert np.array_equal(orc.ancestors(first_all, a, b - a), anc[a:b])
    if name in ("sparse_tiles", "leading_zero_tiles", "carrier@10240", "carrier@2048"):
        assert empty >= 1, "no shard without weight"


@pytest.mark.parametrize("n", [1, 7, 2049, 4097])
def test_zero_total_rule(orc, n):
    """a grand total of 0 gives first[i] = 0 and ancestor n - 1 everywhere; under a gate S = Q = 0 keeps
    the population.  orc_offspring_offsets must not divide: cdf, base and comb_u are handed in at their worst."""
    for name, lw in X.zero_total_cases(n).items():
        wq, total = X.quantised(lw)
        assert total == 0 and not wq.any(), name
        assert np.array_equal(orc.resample(wq, SEED, FRAME), np.full(n, n - 1)), name
        anc, first = X.exact_ancestors(wq, SEED, FRAME)
        assert np.array_equal(anc, np.full(n, n - 1)) and not first.any()
        assert orc.ess_terms(wq) == (0, 0) and not orc.ess_resample(0, 0, n, orc.ess_frac_q16(0.9))
    junk = np.arange(1, n + 1, dtype=np.uint64) << np.uint64(33)
    for total in (0, 1 << 63, (1 << 64) - 1):
        assert not orc.offspring_offsets(junk, 1 << 40, total, 12345, 3 * n).any()
        cnt, first = X.exact_ancestors(junk, SEED, FRAME, n_total=3 * n, base=1 << 40, total=total)
        assert not first.any() and (cnt == n).all()


@pytest.mark.parametrize("n", [7, 2049, 4097])
def test_nan_log_weight_is_a_particle_of_weight_zero(orc, n):
    for name, lw in X.nan_cases(n).items():
        wq, total = X.quantised(lw)
        assert total > 0 and not wq[np.isnan(lw)].any() and wq[~np.isnan(lw)].all(), name
        anc, _ = X.exact_ancestors(wq, SEED, FRAME)
        assert np.array_equal(orc.resample(wq, SEED, FRAME), anc), name
        assert not np.isnan(lw[anc]).any()
