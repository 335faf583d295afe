"""TEST INFRASTRUCTURE: an exact restatement of the systematic resample in Python integers, and a catalogue of
structured weight populations (a single carrier, whole zero tiles, equal runs) with the property each one promises.

The resample: tooth j sits at j * S + u, particle k spans [N * C(k - 1), N * C(k)), so

    ancestor(j) = #{ k in [0, N - 1) : N * C_incl(k) <= j * S + u },
    first[i]    = max(0, ceil((N * C_excl(i) - u) / S)),

with S the grand total, N the number of slots and u = (r64 * S) >> 64 from Philox counter (0, 0, frame, 1).  No division
beyond the one ceil in first[], no floating point, no `first` array on the way to the ancestors; Philox comes from
tests/_f64_pf.py, not from oracle/slam_oracle_pf.c.  A grand total of 0 (or >= 2^63) is pinned to first[i] = 0, and the
formula above then gives ancestor N - 1 for every slot by itself.

The kernels' constants appear here as plain numbers: 2048-element scan tiles, 32-element blocks inside a tile, 256 slots
per workgroup (csrc/resample_common.h: kScanTile; csrc/pf_common.h: kBlock).
"""
import functools
from bisect import bisect_right

import numpy as np

import oracle
from _f64_pf import philox4x32_10

TILE, BLOCK, WG = 2048, 32, 256
CARRIER, ZERO, TINY = np.float32(0.0), np.float32(-200.0), np.float32(-21.5)   # wq = 2^32, 0, a handful of units


def comb_offset(seed, frame, total):
    r = philox4x32_10([0, 0, frame, 1], (seed & 0xFFFFFFFF, seed >> 32))
    r64 = int(r[0]) | (int(r[1]) << 32)
    return (r64 * int(total)) >> 64


def exact_ancestors(wq, seed, frame, n_total=None, base=0, total=None):
    """-> (anc, first) for the particles `wq` (any integers).  Unsharded (the defaults): anc[j] is the ancestor of slot j.
    A shard (n_total slots in all, `base` = the weight in front of it, `total` = the grand total): first[] are the shard's,
    and anc[j], for EVERY slot j of the population, is the number of the shard's particles that lie wholly below tooth j;
    join_shards() adds the shards' counts up to the ancestors."""
    w = [int(v) for v in wq]
    n = len(w)
    whole = n_total is None
    N = n if whole else int(n_total)
    incl, run = [], int(base)
    for v in w:
        run += v
        incl.append(run)
    S = run if total is None else int(total)
    if S == 0 or S >> 63:
        S = u = 0   # the pinned rule: every threshold is 0, every N * C is >= 0
        first = [0] * n
    else:
        u = comb_offset(seed, frame, S)
        first = [max(0, -((u - N * (c - v)) // S)) for c, v in zip(incl, w)]   # ceil((N * C_excl - u) / S), clamped
    if S == 0:
        incl = [0] * n
    scaled = [N * c for c in incl]
    anc = [bisect_right(scaled, j * S + u) for j in range(N)]
    if whole:
        anc = [min(a, n - 1) for a in anc]   # k runs over [0, n - 1): the last particle takes what is left
    return np.array(anc, np.int64), np.array(first, np.int64)


def join_shards(counts, n_total):
    return np.minimum(np.sum(counts, axis=0), n_total - 1)


# ------------------------------------------------------------------ the catalogue


# Promise keys of an entry (broken_promises() checks each on the quantised weights and the reference ancestors):
#   carrier = i           exactly one particle has weight, particle i
#   zero_tiles = [t]      the 2048-element tile t has total weight 0 (equal consecutive tile offsets in the tile-level search)
#   flat_blocks = [b]     "flat": the CDF does not move inside the 32-element block b and equals its predecessor's last value
#                         (equal pivots in the block-level search)
#   carriers_per_tile = c every tile holds exactly c particles with weight
#   wg_span = k           some workgroup of 256 slots has its first and last ancestor k or more tiles apart (more than one
#                         apart is the un-staged branch of ancestors_from_scan_kernel<1>)
#   identity              the ancestors are 0 .. n - 1
#   tiny_max = m          every weight is in [1, m];  below_n: the grand total is in (0, n)
#   dominant = i          particle i has weight 2^32, every other one a weight in [1, 8]
#   equal_run = (a, b)    particles a .. b - 1 carry one weight, their neighbours another, and a < 2048 < b = a + 64
# max (not a promise): the maximum to quantise against where it is not the entry's own (a shard of a larger population).


def _single(n, idx):
    lw = np.full(n, ZERO, np.float32)
    lw[idx] = CARRIER
    return dict(logw=lw, carrier=idx, zero_tiles=[t for t in range((n + TILE - 1) // TILE) if t != idx // TILE],
                flat_blocks=[b for b in range((n + BLOCK - 1) // BLOCK) if b != idx // BLOCK])


def _builders(n):
    """name -> function that makes the entry; the names alone cost nothing (test ids of the large shapes)"""
    ntiles = (n + TILE - 1) // TILE
    out = {}
    spots = {0, n - 1}
    if ntiles >= 2:
        last_edge = (ntiles - 1) * TILE
        spots |= {TILE - 1, TILE, last_edge - 1, last_edge}
    spots |= {i for i in (BLOCK - 1, BLOCK, TILE + BLOCK - 1, TILE + BLOCK) if i < n}
    if ntiles > 256:
        spots.add(256 * TILE + 3)   # alone in the first tile beyond one workgroup's worth of tile offsets
    for i in sorted(spots):
        out[f"carrier@{i}"] = functools.partial(_single, n, i)

    def one_per_tile():
        lw = np.full(n, ZERO, np.float32)
        for t in range(ntiles):
            lw[min(t * TILE + (37 * t + 5) % TILE, n - 1)] = CARRIER
        return dict(logw=lw, carriers_per_tile=1)

    k = max(1, min(2, ntiles - 2))

    def leading():
        lw = np.full(n, CARRIER, np.float32)
        lw[:k * TILE] = ZERO
        return dict(logw=lw, zero_tiles=list(range(k)), flat_blocks=list(range(k * TILE // BLOCK)))

    def trailing():
        lw = np.full(n, CARRIER, np.float32)
        lw[(ntiles - k) * TILE:] = ZERO
        lw[(ntiles - k) * TILE - 1 - BLOCK:(ntiles - k) * TILE - 1] = ZERO   # and a flat stretch in front of a live element
        return dict(logw=lw, zero_tiles=list(range(ntiles - k, ntiles)),
                    flat_blocks=list(range((ntiles - k) * TILE // BLOCK, (n + BLOCK - 1) // BLOCK)))

    def sparse():
        lw = np.full(n, ZERO, np.float32)
        live = list(range(0, ntiles, 4))
        for t in live:
            lw[min(t * TILE + (611 * t + 5) % TILE, n - 1)] = CARRIER
        lw[1:4] = CARRIER   # (unequal shares: the step from tile 0 to tile 4 falls inside a workgroup, not between two)
        return dict(logw=lw, zero_tiles=[t for t in range(ntiles) if t not in live], wg_span=4)

    def tiny_and_sparse():
        lw = np.full(n, ZERO, np.float32)
        lw[2::3] = TINY
        return dict(logw=lw, max=CARRIER, below_n=True)

    def tiny_then_dominant():
        lw = np.full(n, TINY, np.float32)
        lw[n - 1] = CARRIER
        return dict(logw=lw, dominant=n - 1)

    def equal_run():
        a = max(0, min(TILE - 32, n - 64))
        b = min(n, a + 64)
        lw = np.full(n, TINY, np.float32)
        lw[::7] = ZERO
        lw[a:b] = CARRIER
        return dict(logw=lw, equal_run=(a, b))

    if ntiles >= 2:
        out.update(one_per_tile=one_per_tile, leading_zero_tiles=leading, trailing_zero_tiles=trailing)
    if ntiles >= 5:
        out["sparse_tiles"] = sparse
    out["all_equal"] = lambda: dict(logw=np.full(n, CARRIER, np.float32), identity=True)
    # (a population's own maximum quantises to 2^32: the next two are quantised against an outside maximum, as a shard is)
    out["all_tiny"] = lambda: dict(logw=np.full(n, TINY, np.float32), max=CARRIER, tiny_max=8)
    if n >= 3:
        out["tiny_and_sparse"] = tiny_and_sparse
    if n >= 2:
        out["tiny_then_dominant"] = tiny_then_dominant
    if n > TILE:
        out["equal_run_over_tile_edge"] = equal_run
    return out


def names(n):
    """the entries that exist at this n"""
    return list(_builders(n))


def population(n, name):
    """One entry: dict(logw = float32[n], the promise keys above).  Kept for the small shapes, made anew for the large ones."""
    return populations(n)[name] if n <= 1 << 16 else _builders(n)[name]()


@functools.lru_cache(maxsize=None)
def populations(n):
    """name -> entry, for every entry that exists at this n"""
    return {name: make() for name, make in _builders(n).items()}


def quantised(logw, m=None):
    """(wq, grand total) of a log-weight vector as the specification quantises it, against its own maximum (NaN loses
    every maximum) or the given one."""
    lw, own = oracle.logweight(None, logw, 0.0)
    return oracle.quantise_weights(lw, own if m is None else np.float32(m))


def reference(n, name, seed, frame):
    """(wq, total, exact ancestors, exact first) of a catalogue entry: computed once, shared, never written to (the few
    large shapes, each used by one test, are not kept)."""
    return (_reference if n <= 1 << 16 else _reference.__wrapped__)(n, name, seed, frame)


@functools.lru_cache(maxsize=None)
def _reference(n, name, seed, frame):
    entry = population(n, name)
    wq, total = quantised(entry["logw"], entry.get("max"))
    anc, first = exact_ancestors(wq, seed, frame)
    for a in (wq, anc, first):
        a.setflags(write=False)
    return wq, total, anc, first


def broken_promises(entry, wq, anc):
    """What an entry promises and does not keep, as a list of sentences (empty: all kept)."""
    n, bad = len(wq), []
    wq = np.asarray(wq, np.uint64)
    cdf = np.cumsum(wq.astype(object))
    if "carrier" in entry and np.flatnonzero(wq).tolist() != [entry["carrier"]]:
        bad.append("not exactly one carrier at the promised index")
    for t in entry.get("zero_tiles", []):
        if wq[t * TILE:(t + 1) * TILE].any():
            bad.append(f"tile {t} has weight")
    for b in entry.get("flat_blocks", []):
        seg = cdf[b * BLOCK:(b + 1) * BLOCK]
        if len(seg) and seg[0] != seg[-1] or (b > 0 and len(seg) and seg[0] != cdf[b * BLOCK - 1]):
            bad.append(f"the CDF moves inside block {b}")
    if "carriers_per_tile" in entry:
        per = [int(np.count_nonzero(wq[t:t + TILE])) for t in range(0, n, TILE)]
        if set(per) != {entry["carriers_per_tile"]}:
            bad.append("carriers per tile")
    if "wg_span" in entry:
        tiles = np.asarray(anc) // TILE
        span = max(int(tiles[min(j + WG, n) - 1] - tiles[j]) for j in range(0, n, WG))
        if span < entry["wg_span"] or span < 2:
            bad.append(f"no workgroup's slots span {entry['wg_span']} tiles (widest: {span})")
    if entry.get("identity") and not np.array_equal(anc, np.arange(n)):
        bad.append("ancestors are not the identity")
    if entry.get("below_n") and not 0 < int(cdf[-1]) < n:
        bad.append("total is not below n")
    if "tiny_max" in entry and not ((wq > 0) & (wq <= entry["tiny_max"])).all():
        bad.append("weights are not a few units")
    if "dominant" in entry:
        d = entry["dominant"]
        rest = np.delete(wq, d)
        if not (wq[d] == 1 << 32 and (rest > 0).all() and (rest <= 8).all()):
            bad.append("not tiny weights and one dominant particle")
    if "equal_run" in entry:
        a, b = entry["equal_run"]
        if not (b - a == 64 and a < TILE < b and len(set(wq[a:b].tolist())) == 1 and wq[a] > 0 and
                (a == 0 or wq[a - 1] != wq[a]) and (b == n or wq[b] != wq[a])):
            bad.append("no run of 64 equal weights across the tile edge")
    return bad


# ------------------------------------------------------------------ NaN among finite ones, and the zero-total branch


def nan_cases(n):
    """A NaN log-weight is a particle of weight 0: at index 0, at n - 1, as the whole first wavefront of a block."""
    rng = np.random.default_rng(n)
    base = np.where(rng.random(n) < 0.5, CARRIER, TINY).astype(np.float32)
    base[n // 2] = CARRIER
    out = {}
    for name, sel in (("nan@0", slice(0, 1)), ("nan@n-1", slice(n - 1, n)), ("nan_first_wave", slice(0, min(64, n - 1)))):
        lw = base.copy()
        lw[sel] = np.nan
        out[name] = lw
    if n > WG + 64:
        lw = base.copy()
        lw[WG:WG + 64] = np.nan   # the first wavefront of the second workgroup of the weights' launch
        out["nan_first_wave_block1"] = lw
    return out


def zero_total_cases(n):
    """Log-weights whose quantised weights are all 0: the maximum is -inf or +inf, every difference NaN or -inf."""
    inf = np.float32(np.inf)
    one_inf = np.where(np.arange(n) % 3 == 0, np.float32(-1.5), np.float32(0.25)).astype(np.float32)
    one_inf[n // 2] = inf
    only_minus_inf = np.full(n, np.nan, np.float32)
    only_minus_inf[n - 1] = -inf
    return {"all_minus_inf": np.full(n, -inf, np.float32), "all_nan": np.full(n, np.nan, np.float32),
            "one_plus_inf": one_inf, "nan_and_one_minus_inf": only_minus_inf}
