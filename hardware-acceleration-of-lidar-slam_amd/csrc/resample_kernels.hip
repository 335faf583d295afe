// resample_kernels.hip — the systematic resample on one GPU's integer CDF: the ESS gate, the comb's offspring
// offsets (staged, from the tile-local scan, or with the ancestors in the same launch: the owner fills its slots), the ancestor search.
// (The weights: weights_kernels.hip.  The CDF: scan_kernels.hip.  The comb's arithmetic: comb_quotient.h.)
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "block_reduce.h"
#include "comb_quotient.h"
#include "resample_common.h"

namespace slam {

namespace {

// The resample gate (oracle: orc_ess_resample): resample iff ESS < frac * N, i.e. S^2 * 65536 < frac_q16 * N * Q, in
// 128-bit integer arithmetic (S < 2^47, Q < 2^63, N < 2^31, frac_q16 <= 2^16).
__device__ __forceinline__ bool ess_wants_resample(uint64_t s16, uint64_t q16, uint64_t n_total, uint32_t frac_q16)
{
    uint64_t l_lo = s16 * s16, l_hi = __umul64hi(s16, s16);
    l_hi = (l_hi << 16) | (l_lo >> 48);
    l_lo <<= 16;
    const uint64_t nf = n_total * (uint64_t)frac_q16;
    const uint64_t r_lo = q16 * nf, r_hi = __umul64hi(q16, nf);
    return l_hi < r_hi || (l_hi == r_hi && l_lo < r_lo);
}

// verdict of the gate for the rest of the frame loop: a device flag (the next frame's weight kernel reads it) and the
// same value in mapped host memory behind a sequence number (the host picks the EKF form for the next frame)
__device__ __forceinline__ void publish_gate(const GateOut& g, bool resample)
{
    *g.d_flag = resample ? 1 : 0;
    if (g.h_flag) {
        g.h_flag[0] = resample ? 1 : 0;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<uint32_t*>(g.h_flag + 1), g.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

__global__ __launch_bounds__(kBlock) void offspring_offsets_kernel(const uint64_t* __restrict__ cdf, int n,
                                                                   const uint64_t* __restrict__ d_base,
                                                                   const uint64_t* __restrict__ d_total,
                                                                   uint32_t key0, uint32_t key1, uint32_t frame,
                                                                   uint64_t n_total, int32_t* __restrict__ first)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const uint64_t base = d_base ? *d_base : 0ull;
    const uint64_t c_excl = base + (i ? cdf[i - 1] : 0ull);
    first[i] = comb_first(c_excl, *d_total, n_total, key0, key1, frame);
}

// fused form: CDF = base + (sum of earlier tiles) + tile-local scan; every workgroup re-derives its tile's
// offset (and, on a single GPU, the grand total) from the <= n/2048 tile totals instead of a separate pass
__global__ __launch_bounds__(kBlock) void offspring_from_scan_kernel(const uint64_t* __restrict__ cdf_local,
                                                                     const uint64_t* __restrict__ tile_total,
                                                                     int ntiles, int n,
                                                                     const uint64_t* __restrict__ d_base,
                                                                     const uint64_t* __restrict__ d_total,
                                                                     const uint64_t* __restrict__ d_shard_totals,
                                                                     int rank, int world, uint32_t key0,
                                                                     uint32_t key1, uint32_t frame, uint64_t n_total,
                                                                     int32_t* __restrict__ first,
                                                                     const uint64_t* __restrict__ tile_s16,
                                                                     const uint64_t* __restrict__ tile_q16,
                                                                     uint32_t frac_q16, GateOut gate)
{
    __shared__ uint64_t s_red[kBlock / 64];
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int tile = (blockIdx.x * kBlock) / kScanTile;   // kScanTile is a multiple of kBlock
    const bool gated = frac_q16 != 0;
    const int stride = gated ? 3 : 1;   // gated: the ranks all-gather (total, S, Q) triples
    uint64_t before = 0, all = 0, s16 = 0, q16 = 0;
    for (int t = threadIdx.x; t < ntiles; t += kBlock) {
        const uint64_t v = tile_total[t];
        all += v;
        before += t < tile ? v : 0ull;
        if (gated && !d_shard_totals) {
            s16 += tile_s16[t];
            q16 += tile_q16[t];
        }
    }
    before = block_sum_u64(before, s_red);
    uint64_t total, shard_base = d_base ? *d_base : 0ull;
    if (d_shard_totals) {   // several GPUs: the all-gathered shard totals give both the base and the grand total
        total = 0;
        shard_base = 0;
        s16 = q16 = 0;
        for (int q = 0; q < world; ++q) {
            const uint64_t v = d_shard_totals[(size_t)stride * q];
            total += v;
            shard_base += q < rank ? v : 0ull;
            if (gated) {
                s16 += d_shard_totals[3 * (size_t)q + 1];
                q16 += d_shard_totals[3 * (size_t)q + 2];
            }
        }
    } else {
        total = d_total ? *d_total : block_sum_u64(all, s_red);
        if (gated) {
            s16 = block_sum_u64(s16, s_red);
            q16 = block_sum_u64(q16, s_red);
        }
    }
    if (gated) {   // the same verdict in every workgroup and on every rank (integer sums over the whole population)
        const bool resample = ess_wants_resample(s16, q16, n_total, frac_q16);
        if (blockIdx.x == 0 && threadIdx.x == 0) publish_gate(gate, resample);
        if (!resample) {   // every particle keeps its slot: slot j descends from particle j
            if (i < n) first[i] = (int32_t)((int64_t)rank * n + i);
            return;
        }
    }
    if (i >= n) return;
    const uint64_t base = shard_base + before;
    const uint64_t c_excl = base + ((i % kScanTile) ? cdf_local[i - 1] : 0ull);
    first[i] = comb_first(c_excl, total, n_total, key0, key1, frame);
}

// Feedback for the host's choice between the two out-of-place EKF forms (it changes speed, never results): about how many
// DISTINCT ancestors the resample left — `head`: this thread's particle has offspring.  Summed with one atomic per workgroup;
// the workgroup that finishes last hands {count, n} to mapped host memory and clears the counter (8-byte aligned pair of words).
// The host reads it without any synchronisation, a frame or two late.
__device__ __forceinline__ void count_heads(const HeadsOut& h, bool head, int n)
{
    // a sample is enough for a heuristic: every 8th workgroup counts, the result is scaled (same-address atomics run at
    // ~88 per microsecond: one per workgroup cost 14 us at 4096 workgroups)
    if (!h.counter || (blockIdx.x & 7u) != 0) return;
    __shared__ int s_heads[kBlock / 64];
    const int cnt = __popcll(__ballot(head));
    if ((threadIdx.x & 63) == 0) s_heads[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x != 0) return;
    int sum = 0;
    for (int w = 0; w < kBlock / 64; ++w) sum += s_heads[w];
    // ONE 64-bit atomic carries both the count (high word) and the number of workgroups done (low word): nothing else is
    // published, so no fence is needed (a __threadfence() per workgroup made this kernel 2.5x slower at 1M slots)
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(h.counter);
    const unsigned long long old = atomicAdd(acc, ((unsigned long long)(unsigned)sum << 32) | 1ull);
    const unsigned sampled = (gridDim.x + 7u) / 8u;
    if ((unsigned)(old & 0xffffffffu) != sampled - 1) return;
    const long long owners = (long long)sampled * kBlock < n ? (long long)sampled * kBlock : n;   // particles the sample covered (about)
    h.h_out[0] = (int32_t)(((long long)(old >> 32) + sum) * n / owners);
    h.h_out[1] = n;
    atomicExch(acc, 0ull);
}

// Single GPU: the ancestor of every slot straight from the tile-local scan, without materialising `first` and without a
// search: the OWNER fills its slots.  first[i] <= j  <=>  N*C_excl(i) <= j*S + u  (first[i] = ceil((N*C_excl(i) - u)/S),
// clamped at 0), so the ancestor of slot j — the last i with first[i] <= j, the number of k in [0, n-1) with
// N*C_incl(k) <= j*S + u — is i exactly for the slots of [first[i], first[i+1]), and for [first[n-1], n) with the last particle,
// which takes what is left (k stops at n-1).  first[0] = 0 and first[] never falls: the runs tile [0, n).  first[i+1] comes from
// C_incl(i), which IS the neighbour's C_excl (the same sum of the same integers, also across a tile edge: the tile's offset plus
// its total is the next tile's offset), so both bounds come from this thread's own two coalesced loads and no value crosses
// lanes or workgroups.  A total of 0 (or >= 2^63) has first[] = 0 everywhere: every run is empty but the last particle's, the pinned rule
// by itself.  A gated frame that keeps its population: run i is [i, i+1).
// The chain: loads (tile totals and the two CDF values, side by side) -> one block sum -> arithmetic -> stores.
// The fill never loops over a run in one thread: a run of up to kOwnSlots slots is stored by its owner (neighbouring lanes own
// neighbouring slots), a longer one by the whole wavefront, 64 slots per store — at most n/64 + 64 store instructions in a
// wavefront however the weights lie (one particle with all the weight: n/64).
constexpr int kMaxScanTiles = 4096;   // n <= 8M (beyond: the two-launch form)
constexpr int kOwnSlots = 4;
__global__ __launch_bounds__(kBlock) void offspring_fill_kernel(const uint64_t* __restrict__ cdf_local,
                                                                const uint64_t* __restrict__ tile_total, int ntiles, int n,
                                                                uint32_t key0, uint32_t key1, uint32_t frame,
                                                                int32_t* __restrict__ anc, const uint64_t* __restrict__ tile_s16,
                                                                const uint64_t* __restrict__ tile_q16, uint32_t frac_q16,
                                                                GateOut gate, HeadsOut heads, SurvivorOut survivors)
{
    __shared__ uint64_t s_red[4][kBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x * kBlock + threadIdx.x;      // the particle this thread owns
    const int tile = (blockIdx.x * kBlock) / kScanTile;   // kScanTile is a multiple of kBlock
    const bool in = i < n, gated = frac_q16 != 0;
    const uint64_t c_own = in ? cdf_local[i] : 0ull;                           // inclusive, local to the tile
    const uint64_t c_prev = in && (i % kScanTile) ? cdf_local[i - 1] : 0ull;   // exclusive: 0 at a tile's start
    uint64_t before = 0, total = 0, s16 = 0, q16 = 0;
    for (int t = threadIdx.x; t < ntiles; t += kBlock) {   // (one turn up to 512k particles)
        const uint64_t v = tile_total[t];
        total += v;
        before += t < tile ? v : 0ull;
        if (gated) {
            s16 += tile_s16[t];
            q16 += tile_q16[t];
        }
    }
    // (not four block_sum_u64: ONE barrier for the four sums on the chain above — a choice, not a copy)
    before = wave_sum_u64(before);
    total = wave_sum_u64(total);
    if (gated) {
        s16 = wave_sum_u64(s16);
        q16 = wave_sum_u64(q16);
    }
    if (lane == 0) {
        s_red[0][wave] = before;
        s_red[1][wave] = total;
        s_red[2][wave] = s16;
        s_red[3][wave] = q16;
    }
    __syncthreads();
    before = total = s16 = q16 = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        before += s_red[0][w];
        total += s_red[1][w];
        s16 += s_red[2][w];
        q16 += s_red[3][w];
    }
    bool resample = true;
    if (gated) {   // resample gate: the same verdict in every workgroup
        resample = ess_wants_resample(s16, q16, (uint64_t)n, frac_q16);
        if (blockIdx.x == 0 && threadIdx.x == 0) publish_gate(gate, resample);
    }
    int lo = i, hi = i + 1;   // the frame keeps its population: slot i descends from particle i
    if (resample) {
        // comb_total_unusable() and comb_draw() (comb_quotient.h) written out, the draw once for both bounds: called, they let the
        // compiler order this kernel's instructions differently, and the frame path keeps its instruction stream
        lo = hi = 0;   // an unusable total: first[] = 0
        if (!(total == 0 || (total >> 63))) {
            const u32x4 r = philox4x32_10(0u, 0u, frame, 1u /* resample stream */, key0, key1);
            const uint64_t comb_u = __umul64hi((uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32), total);
            lo = comb_first_quick(before + c_prev, total, (uint64_t)n, comb_u);
            hi = comb_first_quick(before + c_own, total, (uint64_t)n, comb_u);
        }
        if (i == n - 1) hi = n;   // the last particle takes every slot that is left
        lo = lo < 0 ? 0 : lo > n ? n : lo;
        hi = hi < 0 ? 0 : hi > n ? n : hi;
    }
    if (!in) lo = hi = 0;
    const int len = hi - lo;
#pragma unroll
    for (int k = 0; k < kOwnSlots; ++k)
        if (len <= kOwnSlots && k < len) anc[lo + k] = i;
    for (unsigned long long wide = __ballot(len > kOwnSlots); wide; wide &= wide - 1) {
        const int src = __ffsll(wide) - 1;   // (wavefront-uniform: the run's bounds come through scalar registers)
        const int r_lo = __builtin_amdgcn_readlane(lo, src), r_hi = __builtin_amdgcn_readlane(hi, src);
        const int owner = i - lane + src;
        for (int s = r_lo + lane; s < r_hi; s += 64) anc[s] = owner;
    }
    // survivor rows: the particles this resample kept mark themselves
    if (len > 0 && survivors.mark) survivors.mark[i] = survivors.stamp;
    count_heads(heads, len > 0, n);
}

__global__ __launch_bounds__(kBlock) void ancestors_kernel(const int32_t* __restrict__ first_all, int64_t n_total,
                                                           int64_t slot0, int nslots, int32_t* __restrict__ anc)
{
    const int s = blockIdx.x * kBlock + threadIdx.x;
    if (s >= nslots) return;
    anc[s] = (int32_t)last_with_first_le(first_all, n_total, slot0 + s);
}

}  // namespace

hipError_t launch_offspring_from_scan(hipStream_t stream, const uint64_t* cdf_local, const uint64_t* tile_total, int n,
                                      const uint64_t* d_base, const uint64_t* d_total, const uint64_t* d_shard_totals,
                                      int rank, int world, uint64_t seed, uint32_t frame, int64_t n_total,
                                      int32_t* first, uint32_t frac_q16, const GateOut& gate)
{
    if (n <= 0) return hipSuccess;
    const int ntiles = scan_tile_count(n);
    offspring_from_scan_kernel<<<blocks_for(n), kBlock, 0, stream>>>(cdf_local, tile_total, ntiles, n, d_base, d_total,
                                                                     d_shard_totals, rank, world, (uint32_t)seed,
                                                                     (uint32_t)(seed >> 32), frame, (uint64_t)n_total,
                                                                     first, tile_total + ntiles, tile_total + 2 * ntiles,
                                                                     frac_q16, gate);
    return hipGetLastError();
}

hipError_t launch_offspring_offsets(hipStream_t stream, const uint64_t* cdf, int n, const uint64_t* d_base,
                                    const uint64_t* d_total, uint64_t seed, uint32_t frame, int64_t n_total,
                                    int32_t* first)
{
    if (n <= 0) return hipSuccess;
    offspring_offsets_kernel<<<blocks_for(n), kBlock, 0, stream>>>(cdf, n, d_base, d_total, (uint32_t)seed,
                                                                   (uint32_t)(seed >> 32), frame, (uint64_t)n_total,
                                                                   first);
    return hipGetLastError();
}

bool ancestors_from_scan_fits(int n) { return n > 0 && scan_tile_count(n) <= kMaxScanTiles; }

hipError_t launch_ancestors_from_scan(hipStream_t stream, const uint64_t* cdf_local, const uint64_t* tile_total, int n,
                                      uint64_t seed, uint32_t frame, int32_t* anc, uint32_t frac_q16, const GateOut& gate,
                                      const HeadsOut& heads, const SurvivorOut& survivors)
{
    if (n <= 0) return hipSuccess;
    const int ntiles = scan_tile_count(n);
    const uint64_t *ts = tile_total + ntiles, *tq = tile_total + 2 * ntiles;   // layout of the engine's scan state
    offspring_fill_kernel<<<blocks_for(n), kBlock, 0, stream>>>(cdf_local, tile_total, ntiles, n, (uint32_t)seed, (uint32_t)(seed >> 32),
                                                                frame, anc, ts, tq, frac_q16, gate, heads, survivors);
    return hipGetLastError();
}

hipError_t launch_ancestors(hipStream_t stream, const int32_t* first_all, int64_t n_total, int64_t slot0, int nslots,
                            int32_t* anc)
{
    if (nslots <= 0) return hipSuccess;
    ancestors_kernel<<<blocks_for(nslots), kBlock, 0, stream>>>(first_all, n_total, slot0, nslots, anc);
    return hipGetLastError();
}

}  // namespace slam
