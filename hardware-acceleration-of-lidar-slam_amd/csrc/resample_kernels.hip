// resample_kernels.hip — weights and resampling on one GPU: log-weights (with the covariance classes'
// update riding along; behind the scan's tiles instead on a frame whose front launch made the weights), maximum, quantise, tile scan, ESS gate, offspring offsets, ancestors; and the small result and gather
// kernels that use the same block reductions (arg-max, best particle, pose sums, gather_f32, gather_map).
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "det_math.h"
#include "comb_quotient.h"
#include "cov_update_body.h"
#include "pf_common.h"

namespace slam {

namespace {

// ------------------------------------------------------------------ A11: weights
// (log_weight_of, wave_max: pf_common.h)
// carry (optional): the normalised log-weights the previous frame left behind; they count only when that frame did
// NOT resample (*prev_resampled == 0, a device flag written by the previous frame's resample kernel)
__global__ __launch_bounds__(kBlock) void logweight_kernel(const float* __restrict__ score,
                                                           const float* __restrict__ loglik, float gain, int n,
                                                           const float* __restrict__ carry,
                                                           const int32_t* __restrict__ prev_resampled,
                                                           float* __restrict__ logw, float* __restrict__ block_max)
{
    __shared__ float s_max[kBlock / 64];
    float m = -INFINITY;
    const bool add_carry = carry && *prev_resampled == 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float ll = loglik ? loglik[i] : 0.0f;
        const float sc = score ? score[i] * gain : 0.0f;
        const float lw = log_weight_of(ll, sc, carry, add_carry, i);
        logw[i] = lw;
        m = lw > m ? lw : m;
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = fmaxf(m, s_max[w]);
        block_max[blockIdx.x] = m;
    }
}

// The same launch with the covariance classes' update of a split session in workgroups of its own behind the first `nw`
// (cov_update_body.h): the two have nothing to do with each other — which is the point, they need no launch each.
__global__ __launch_bounds__(kBlock) void logweight_cov_kernel(const float* __restrict__ score, const float* __restrict__ loglik,
                                                               float gain, int n, const float* __restrict__ carry,
                                                               const int32_t* __restrict__ prev_resampled, float* __restrict__ logw,
                                                               float* __restrict__ block_max, int nw, int ly, CovArgs cov)
{
    if ((int)blockIdx.x >= nw) {
        const int j = (int)blockIdx.x - nw;
        cov_update_body(cov, j / ly, j % ly);
        return;
    }
    __shared__ float s_max[kBlock / 64];
    float m = -INFINITY;
    const bool add_carry = carry && *prev_resampled == 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += nw * kBlock) {
        const float ll = loglik ? loglik[i] : 0.0f;
        const float sc = score ? score[i] * gain : 0.0f;
        const float lw = log_weight_of(ll, sc, carry, add_carry, i);
        logw[i] = lw;
        m = lw > m ? lw : m;
    }
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = fmaxf(m, s_max[w]);
        block_max[blockIdx.x] = m;
    }
}

// Several GPUs: the maximum of the block maxima as one float for the all-reduce.  (Folding this into the kernel above with
// a "last workgroup done" ticket was measured and dropped: two atomics per workgroup on one address run at ~88 per
// microsecond, 47 us at 2048 workgroups against 5 us for this launch.)
__global__ __launch_bounds__(kBlock) void max_finalize_kernel(const float* __restrict__ block_max, int nblocks,
                                                              float* __restrict__ d_max)
{
    __shared__ float s_max[kBlock / 64];
    float m = -INFINITY;
    for (int i = threadIdx.x; i < nblocks; i += kBlock) m = fmaxf(m, block_max[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) m = fmaxf(m, s_max[w]);
        *d_max = m;
    }
}

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

__global__ __launch_bounds__(kBlock) void quantise_weights_kernel(const float* __restrict__ logw,
                                                                  const float* __restrict__ d_max, int n,
                                                                  uint64_t* __restrict__ wq,
                                                                  unsigned long long* __restrict__ d_sum)
{
    __shared__ uint64_t s_sum[kBlock / 64];
    const float m = *d_max;
    uint64_t acc = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const float w = det_expf(logw[i] - m);
        const uint64_t q = (uint64_t)(w * 4294967296.0f);
        wq[i] = q;
        acc += q;
    }
    acc = wave_sum_u64(acc);
    if ((threadIdx.x & 63) == 0) s_sum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBlock / 64; ++w) acc += s_sum[w];
        atomicAdd(d_sum, (unsigned long long)acc);   // integer: exact and order-independent
    }
}

// ------------------------------------------------------------------ A12: integer CDF, comb, ancestors
constexpr int kScanItems = 8;                       // elements per thread
constexpr int kScanTile = kBlock * kScanItems;      // 2048 elements per workgroup

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d)
{
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

// inclusive scan of one value per thread over the workgroup: wavefront scan + carry through LDS
__device__ __forceinline__ uint64_t block_inclusive_scan(uint64_t v, uint64_t* s_wave /*[kBlock/64]*/, uint64_t& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t up = shfl_up_u64(v, d);
        if (lane >= d) v += up;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    uint64_t carry = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) carry += s_wave[w];
        tot += s_wave[w];
    }
    total = tot;
    __syncthreads();
    return v + carry;
}

__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(const uint64_t* __restrict__ in, int n,
                                                            uint64_t* __restrict__ out,
                                                            uint64_t* __restrict__ tile_total)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    const int base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
    uint64_t v[kScanItems];
    uint64_t run = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k;
        run += i < n ? in[i] : 0;
        v[k] = run;
    }
    uint64_t total;
    const uint64_t incl = block_inclusive_scan(run, s_wave, total);
    const uint64_t excl = incl - run;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k;
        if (i < n) out[i] = v[k] + excl;
    }
    if (threadIdx.x == 0) tile_total[blockIdx.x] = total;
}

// exclusive scan of the tile totals, in place, by ONE workgroup (<= a few thousand tiles)
__global__ __launch_bounds__(kBlock) void scan_totals_kernel(uint64_t* __restrict__ tile_total, int ntiles)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    uint64_t carry = 0;
    for (int t0 = 0; t0 < ntiles; t0 += kBlock) {
        const int t = t0 + threadIdx.x;
        const uint64_t v = t < ntiles ? tile_total[t] : 0;
        uint64_t total;
        const uint64_t incl = block_inclusive_scan(v, s_wave, total);
        if (t < ntiles) tile_total[t] = carry + incl - v;
        carry += total;
    }
}

__global__ __launch_bounds__(kBlock) void add_tile_offsets_kernel(uint64_t* __restrict__ out, int n,
                                                                  const uint64_t* __restrict__ tile_excl)
{
    const uint64_t off = tile_excl[blockIdx.x];
    const int base = blockIdx.x * kScanTile + threadIdx.x * kScanItems;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k;
        if (i < n) out[i] += off;
    }
}

// ---- fused frame-loop form: weights are quantised and scanned in one pass, never stored
// max over an array of block maxima, by the whole workgroup (every workgroup repeats it: <= 2048 floats)
__device__ __forceinline__ float block_max_of(const float* __restrict__ v, int count, float* s_red /*[kBlock/64]*/)
{
    float m = -INFINITY;
    for (int i = threadIdx.x; i < count; i += kBlock) m = fmaxf(m, v[i]);
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = s_red[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) r = fmaxf(r, s_red[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* s_red /*[kBlock/64]*/)
{
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) r += s_red[w];
    __syncthreads();
    return r;
}

// GATED: also what the resample gate needs — the 16-bit weight sums S = sum(wq >> 16), Q = sum((wq >> 16)^2) of the
// tile (exact integers, hence independent of order and sharding) and carry[i] = logw[i] - max, the weight a particle
// takes into the next frame when this one does not resample (oracle: orc_ess_terms / orc_weight_carry).
// tile `tile` of `ntiles`, by one workgroup (quantise_scan_kernel: the whole grid; quantise_scan_cov_kernel: its first part)
template <bool GATED>
__device__ __forceinline__ void quantise_scan_body(const float* __restrict__ logw, const float* __restrict__ d_max,
                                                   const float* __restrict__ block_max, int nblock_max, int n,
                                                   uint64_t* __restrict__ cdf_local, uint64_t* __restrict__ tile_total,
                                                   float* __restrict__ carry, uint64_t* __restrict__ tile_s16,
                                                   uint64_t* __restrict__ tile_q16, uint64_t* __restrict__ d_sum,
                                                   unsigned int* __restrict__ ticket, unsigned tile, unsigned ntiles)
{
    __shared__ uint64_t s_wave[kBlock / 64];
    __shared__ float s_red[kBlock / 64];
    const int base = tile * kScanTile + threadIdx.x * kScanItems;
    float lw[kScanItems];   // asked for in front of the maximum's reduction and its two barriers, which they do not need
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) lw[k] = base + k < n ? logw[base + k] : 0.0f;
    const float m = d_max ? *d_max : block_max_of(block_max, nblock_max, s_red);
    uint64_t v[kScanItems];
    uint64_t run = 0, s16 = 0, q16 = 0;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k;
        uint64_t q = 0;
        if (i < n) {
            const float rel = lw[k] - m;
            q = (uint64_t)(det_expf(rel) * 4294967296.0f);
            if (GATED) carry[i] = rel;
        }
        run += q;
        v[k] = run;
        if (GATED) {
            const uint64_t w = q >> 16;
            s16 += w;
            q16 += w * w;
        }
    }
    uint64_t total;
    const uint64_t incl = block_inclusive_scan(run, s_wave, total);
    const uint64_t excl = incl - run;
#pragma unroll
    for (int k = 0; k < kScanItems; ++k) {
        const int i = base + k;
        if (i < n) cdf_local[i] = v[k] + excl;   // inclusive, local to this 2048-element tile
    }
    if (threadIdx.x == 0) tile_total[tile] = total;
    if (GATED) {
        s16 = wave_sum_u64(s16);
        q16 = wave_sum_u64(q16);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = s16;
        __syncthreads();
        uint64_t a = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) a += s_wave[w];
        __syncthreads();
        if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = q16;
        __syncthreads();
        uint64_t b = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) b += s_wave[w];
        if (threadIdx.x == 0) {
            tile_s16[tile] = a;
            tile_q16[tile] = b;
        }
    }
    if (!d_sum || threadIdx.x != 0) return;
    // several GPUs: the shard's sums (what the ranks all-gather) through integer atomics; the ticket add depends on their
    // return values, so it is issued only after they have landed; the workgroup that finishes last hands the sums over and
    // clears the accumulators.  No fences: nothing but atomics is published (a release fence per workgroup — an L2
    // write-back across the XCDs — made this kernel 33 instead of 12 us at 512 workgroups).  Saves the one-workgroup launch
    // behind this kernel at the usual shard sizes (32 workgroups at 64k particles).
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(ticket + 2);   // 3 accumulators behind the ticket
    unsigned long long dep = atomicAdd(&acc[0], (unsigned long long)total);
    if (GATED) {
        dep ^= atomicAdd(&acc[1], (unsigned long long)tile_s16[tile]);
        dep ^= atomicAdd(&acc[2], (unsigned long long)tile_q16[tile]);
    }
    uint32_t one = 1u;
    asm volatile("" : "+v"(one) : "v"(dep));
    if (atomicAdd(&ticket[0], one) != ntiles - 1) return;
    for (int a = 0; a < (GATED ? 3 : 1); ++a) d_sum[a] = atomicExch(&acc[a], 0ull);
    ticket[0] = 0;
}

template <bool GATED>
__global__ __launch_bounds__(kBlock) void quantise_scan_kernel(const float* __restrict__ logw,
                                                               const float* __restrict__ d_max,
                                                               const float* __restrict__ block_max, int nblock_max,
                                                               int n, uint64_t* __restrict__ cdf_local,
                                                               uint64_t* __restrict__ tile_total,
                                                               float* __restrict__ carry,
                                                               uint64_t* __restrict__ tile_s16,
                                                               uint64_t* __restrict__ tile_q16,
                                                               uint64_t* __restrict__ d_sum,
                                                               unsigned int* __restrict__ ticket)
{
    quantise_scan_body<GATED>(logw, d_max, block_max, nblock_max, n, cdf_local, tile_total, carry, tile_s16, tile_q16, d_sum, ticket,
                              blockIdx.x, gridDim.x);
}

// The ungated scan with the covariance classes' update of a split session in workgroups of its own behind the `ntiles` tiles
// (cov_update_body.h), as logweight_cov_kernel carries it: on a frame whose front launch has made the weights itself
// (frame_particle_kernel, front_kernels.hip) there is no weights' launch for it to ride in.
__global__ __launch_bounds__(kBlock) void quantise_scan_cov_kernel(const float* __restrict__ logw, const float* __restrict__ block_max,
                                                                   int nblock_max, int n, uint64_t* __restrict__ cdf_local,
                                                                   uint64_t* __restrict__ tile_total, uint64_t* __restrict__ d_sum,
                                                                   unsigned int* __restrict__ ticket, int ntiles, int ly, CovArgs cov)
{
    if ((int)blockIdx.x >= ntiles) {
        const int j = (int)blockIdx.x - ntiles;
        cov_update_body(cov, j / ly, j % ly);
        return;
    }
    quantise_scan_body<false>(logw, nullptr, block_max, nblock_max, n, cdf_local, tile_total, nullptr, nullptr, nullptr, d_sum, ticket,
                              blockIdx.x, (unsigned)ntiles);
}

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

// floor((hi:lo) / d) for hi < d < 2^63 (so the quotient fits 64 bits): restoring long division
__device__ __forceinline__ uint64_t div128by64(uint64_t hi, uint64_t lo, uint64_t d)
{
    uint64_t rem = hi, q = 0;
#pragma unroll 8
    for (int b = 63; b >= 0; --b) {
        rem = (rem << 1) | ((lo >> b) & 1ull);
        if (rem >= d) {
            rem -= d;
            q |= 1ull << b;
        }
    }
    return q;
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
    const uint64_t total = *d_total;
    if (total == 0 || (total >> 63)) {   // impossible with finite log-weights (the best particle has wq = 2^32);
        first[i] = 0;                    // stay memory-safe anyway: no division, every slot gets the last particle
        return;
    }
    // comb offset u in [0,total): Philox counter (0,0,frame,1), high 64 bits of r64*total (wave-uniform)
    const u32x4 r = philox4x32_10(0u, 0u, frame, 1u /* resample stream */, key0, key1);
    const uint64_t comb_u = __umul64hi((uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32), total);
    const uint64_t c_excl = base + (i ? cdf[i - 1] : 0ull);
    // X = c_excl * n_total as 128 bits
    uint64_t lo = c_excl * n_total, hi = __umul64hi(c_excl, n_total);
    int32_t f = 0;
    if (hi != 0 || lo > comb_u) {
        // (X - u - 1) / total + 1
        const uint64_t sub = comb_u + 1ull;   // comb_u < total < 2^63: no overflow
        hi -= lo < sub ? 1ull : 0ull;
        lo -= sub;
        f = (int32_t)(div128by64(hi, lo, total) + 1ull);
    }
    first[i] = f;
}

// comb_first(): shared by the staged and the fused offsets kernels
__device__ __forceinline__ int32_t comb_first(uint64_t c_excl, uint64_t total, uint64_t n_total, uint32_t key0,
                                              uint32_t key1, uint32_t frame)
{
    if (total == 0 || (total >> 63)) return 0;   // see offspring_offsets_kernel
    const u32x4 r = philox4x32_10(0u, 0u, frame, 1u /* resample stream */, key0, key1);
    const uint64_t comb_u = __umul64hi((uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32), total);
    uint64_t lo = c_excl * n_total, hi = __umul64hi(c_excl, n_total);
    if (hi == 0 && lo <= comb_u) return 0;
    const uint64_t sub = comb_u + 1ull;
    hi -= lo < sub ? 1ull : 0ull;
    lo -= sub;
    return (int32_t)(div128by64(hi, lo, total) + 1ull);
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

// first[] of a particle whose exclusive CDF is c, with the comb offset already drawn and the total known to be sane
// (comb_first() without its 64-step division: the offset sits on the one dependent chain of offspring_fill_kernel)
__device__ __forceinline__ int32_t comb_first_quick(uint64_t c, uint64_t total, uint64_t n_total, uint64_t comb_u)
{
    uint64_t lo = c * n_total, hi = __umul64hi(c, n_total);
    if (hi == 0 && lo <= comb_u) return 0;
    const uint64_t sub = comb_u + 1ull;
    hi -= lo < sub ? 1ull : 0ull;
    lo -= sub;
    return (int32_t)(quotient_below_2_32(hi, lo, total) + 1ull);   // c <= total: at most n_total
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
        lo = hi = 0;   // total 0 or >= 2^63 (see offspring_offsets_kernel): no division, first[] = 0
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
    const int64_t j = slot0 + s;
    int64_t lo = 0, hi = n_total;   // first index whose first slot is > j
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)first_all[mid] <= j) lo = mid + 1; else hi = mid;
    }
    anc[s] = (int32_t)(lo - 1);
}

// ------------------------------------------------------------------ results and gathers
__global__ __launch_bounds__(kBlock) void gather_f32_kernel(const float* __restrict__ src,
                                                            const int32_t* __restrict__ idx, int n,
                                                            float* __restrict__ dst)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}

// out row i = in row idx[i]; one workgroup per particle
__global__ __launch_bounds__(kBlock) void gather_map_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                            int64_t in_row_stride, int64_t out_row_stride,
                                                            int in_plane_stride, int out_plane_stride,
                                                            int nlandmarks, const int32_t* __restrict__ idx, int n)
{
    const int i = blockIdx.x;
    if (i >= n) return;
    const float* __restrict__ src = in + (int64_t)idx[i] * in_row_stride;
    float* __restrict__ dst = out + (int64_t)i * out_row_stride;
    for (int pl = 0; pl < 5; ++pl)
        for (int l = threadIdx.x; l < nlandmarks; l += kBlock) dst[pl * out_plane_stride + l] = src[pl * in_plane_stride + l];
}

// index of the largest value, lowest index on ties, NaN never wins (the heaviest particle); one workgroup
__global__ __launch_bounds__(1024) void argmax_kernel(const float* __restrict__ v, int n, int32_t* __restrict__ idx_out,
                                                      float* __restrict__ val_out)
{
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float x = v[i];
        if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 16; ++w)
            if (s_v[w] > bv || (s_v[w] == bv && s_i[w] < bi)) { bv = s_v[w]; bi = s_i[w]; }
        *idx_out = bv > -INFINITY ? bi : 0;   // nothing but -inf and NaN: particle 0
        *val_out = bv;
    }
}

// The heaviest particle with its pose, in one launch: {logw, global id, x, y, theta} to device memory and, optionally,
// to mapped host memory behind a sequence number (a plain C host then needs no copy and no stream synchronisation).
__global__ __launch_bounds__(1024) void best_particle_kernel(const float* __restrict__ v, int n,
                                                             const float* __restrict__ px, const float* __restrict__ py,
                                                             const float* __restrict__ pth, int64_t first_id,
                                                             float* __restrict__ out5, float* __restrict__ h_out5,
                                                             uint32_t* __restrict__ h_seq, uint32_t seq)
{
    __shared__ float s_v[16];
    __shared__ int s_i[16];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float x = v[i];
        if (x > bv || (x == bv && i < bi)) { bv = x; bi = i; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o);
        const int oi = __shfl_xor(bi, o);
        if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = bv; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x != 0) return;
    for (int w = 1; w < 16; ++w)
        if (s_v[w] > bv || (s_v[w] == bv && s_i[w] < bi)) { bv = s_v[w]; bi = s_i[w]; }
    if (!(bv > -INFINITY)) bi = 0;   // nothing but -inf and NaN: particle 0
    const float r[5] = { bv, __int_as_float((int32_t)(first_id + bi)), px[bi], py[bi], pth[bi] };
    for (int k = 0; k < 5; ++k) out5[k] = r[k];
    if (h_out5) {
        for (int k = 0; k < 5; ++k) h_out5[k] = r[k];
        __threadfence_system();
        __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// Exact, order-independent sums over the population for the posterior mean: x and y as 2^-32 fixed point, the heading
// as sin / cos of (theta - ref) in 2^-30 fixed point (det_sincosf: the specified polynomial), accumulated with 64-bit
// integer atomics — the same bits for any summation order, workgroup count or sharding.  idx (optional): the pending
// resample gather.  The last workgroup to finish (a ticket) hands the sums over — to device memory and,
// optionally, mapped host memory behind a sequence number — and clears the accumulators for the next call.
// WEIGHTED (a frame the resample gate kept): slot i counts with the 16-bit weight the gate's S is made
// of, w16 = quantise(det_exp(carry[i])) >> 16 <= 2^16.  The products pass 64 bits, so every value V goes in as two limbs,
// w16 * (V >> 21) and w16 * (V & 0x1fffff): nine sums {x hi, x lo, y hi, y lo, sin hi, sin lo, cos hi, cos lo, sum w16}.
// |V| <= 2^42 (|x|, |y| <= 1024 m) keeps a limb product below 2^37, and 2^23 of them below 2^60.
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void pose_sums_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                           const float* __restrict__ th, const int32_t* __restrict__ idx,
                                                           const float* __restrict__ carry, int n, float ref_th,
                                                           unsigned long long* __restrict__ acc,
                                                           unsigned int* __restrict__ ticket, long long* __restrict__ out,
                                                           long long* __restrict__ h_out, uint32_t* __restrict__ h_seq,
                                                           uint32_t seq)
{
    constexpr int kSums = WEIGHTED ? kPoseSumsWeighted : kPoseSumsPlain;
    __shared__ uint64_t s_red[kBlock / 64];
    uint64_t sum[kSums];   // two's complement: signed sums through unsigned adds
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int j = idx ? idx[i] : i;
        float s, c;
        det_sincosf(th[j] - ref_th, s, c);
        const long long v[4] = { (long long)(x[j] * 4294967296.0f), (long long)(y[j] * 4294967296.0f),
                                 (long long)(s * 1073741824.0f), (long long)(c * 1073741824.0f) };
        if (WEIGHTED) {
            const long long w = (long long)((uint64_t)(det_expf(carry[i]) * 4294967296.0f) >> 16);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                sum[2 * k] += (uint64_t)(w * (v[k] >> 21));
                sum[2 * k + 1] += (uint64_t)(w * (v[k] & 0x1fffffll));
            }
            sum[8] += (uint64_t)w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) sum[k] += (uint64_t)v[k];
        }
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k) sum[k] = block_sum_u64(sum[k], s_red);
    if (threadIdx.x != 0) return;
#pragma unroll
    for (int k = 0; k < kSums; ++k) atomicAdd(&acc[k], (unsigned long long)sum[k]);
    __threadfence();
    if (atomicAdd(ticket, 1u) != gridDim.x - 1) return;
    __threadfence();
    long long r[kSums];
    for (int k = 0; k < kSums; ++k) r[k] = (long long)atomicExch(&acc[k], 0ull);   // read and clear for the next call
    *ticket = 0;
    for (int k = 0; k < kSums; ++k) out[k] = r[k];
    if (h_out) {
        for (int k = 0; k < kSums; ++k) h_out[k] = r[k];
        __threadfence_system();
        __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

static int capped_blocks(int n) { const int b = blocks_for(n); return b < kMaxWeightBlocks ? b : kMaxWeightBlocks; }
int logweight_scratch_elems(int n) { return capped_blocks(n > 0 ? n : 1); }
int logweight_scratch_floats() { return kMaxWeightBlocks + 2; }   // block maxima + {ticket, running maximum} (zero-initialise once)

hipError_t launch_logweight(hipStream_t stream, const float* score, const float* loglik, float gain, int n,
                            float* logw, float* block_max_scratch, float* d_max, const float* carry,
                            const int32_t* prev_resampled, const CovArgs* cov, int cov_bound)
{
    if (n <= 0) return hipSuccess;
    const int nb = capped_blocks(n);
    if (cov && cov_bound > 0) {   // + the covariance classes' update (a grid of cov_bound x ly workgroups, flattened)
        const int ly = cov->nlandmarks > 0 ? (cov->nlandmarks + 255) / 256 : 1;
        logweight_cov_kernel<<<nb + (int64_t)cov_bound * ly, kBlock, 0, stream>>>(score, loglik, gain, n, carry, prev_resampled, logw,
                                                                               block_max_scratch, nb, ly, *cov);
    } else
        logweight_kernel<<<nb, kBlock, 0, stream>>>(score, loglik, gain, n, carry, prev_resampled, logw, block_max_scratch);
    if (d_max) max_finalize_kernel<<<1, kBlock, 0, stream>>>(block_max_scratch, nb, d_max);
    return hipGetLastError();
}

hipError_t launch_quantise_weights(hipStream_t stream, const float* logw, const float* d_max, int n, uint64_t* wq,
                                   uint64_t* d_sum)
{
    hipError_t err = hipMemsetAsync(d_sum, 0, sizeof(uint64_t), stream);
    if (err != hipSuccess) return err;
    if (n <= 0) return hipSuccess;
    quantise_weights_kernel<<<capped_blocks(n), kBlock, 0, stream>>>(logw, d_max, n, wq,
                                                                     reinterpret_cast<unsigned long long*>(d_sum));
    return hipGetLastError();
}

int scan_tile_count(int n) { return (n + kScanTile - 1) / kScanTile; }
int prefix_sum_scratch_elems(int n) { return scan_tile_count(n) + 1; }

hipError_t launch_prefix_sum(hipStream_t stream, const uint64_t* in, int n, uint64_t* out, uint64_t* block_scratch)
{
    if (n <= 0) return hipSuccess;
    const int ntiles = scan_tile_count(n);
    scan_tiles_kernel<<<ntiles, kBlock, 0, stream>>>(in, n, out, block_scratch);
    if (ntiles > 1) {
        scan_totals_kernel<<<1, kBlock, 0, stream>>>(block_scratch, ntiles);
        add_tile_offsets_kernel<<<ntiles, kBlock, 0, stream>>>(out, n, block_scratch);
    }
    return hipGetLastError();
}

hipError_t launch_quantise_scan(hipStream_t stream, const float* logw, const float* d_max, const float* block_max,
                                int nblock_max, int n, uint64_t* cdf_local, uint64_t* tile_total, uint64_t* d_sum,
                                float* carry, uint64_t* tile_s16, uint64_t* tile_q16, unsigned int* ticket, const CovArgs* cov,
                                int cov_bound)
{
    if (n <= 0) return hipSuccess;
    const int ntiles = scan_tile_count(n);
    if (cov && cov_bound > 0) {   // + the covariance classes' update (cov_bound x ly workgroups, flattened, as launch_logweight's)
        if (carry || d_max) return hipErrorInvalidValue;   // the rider exists for the ungated scan over block maxima only
        const int ly = cov->nlandmarks > 0 ? (cov->nlandmarks + 255) / 256 : 1;
        quantise_scan_cov_kernel<<<ntiles + (int64_t)cov_bound * ly, kBlock, 0, stream>>>(logw, block_max, nblock_max, n, cdf_local,
                                                                                        tile_total, d_sum, ticket, ntiles, ly, *cov);
        return hipGetLastError();
    }
    // `ticket`: {ticket, pad, three 64-bit accumulators} (8-byte aligned behind the pad), zero-initialised, left zeroed
    if (carry)
        quantise_scan_kernel<true><<<ntiles, kBlock, 0, stream>>>(logw, d_max, block_max, nblock_max, n, cdf_local, tile_total,
                                                                  carry, tile_s16, tile_q16, d_sum, ticket);
    else
        quantise_scan_kernel<false><<<ntiles, kBlock, 0, stream>>>(logw, d_max, block_max, nblock_max, n, cdf_local,
                                                                   tile_total, nullptr, nullptr, nullptr, d_sum, ticket);
    return hipGetLastError();
}

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

hipError_t launch_argmax(hipStream_t stream, const float* v, int n, int32_t* idx_out, float* val_out)
{
    if (n <= 0) return hipSuccess;
    argmax_kernel<<<1, 1024, 0, stream>>>(v, n, idx_out, val_out);
    return hipGetLastError();
}

hipError_t launch_best_particle(hipStream_t stream, const float* v, int n, const float* px, const float* py,
                                const float* pth, int64_t first_id, float* out5, float* h_out5, uint32_t* h_seq,
                                uint32_t seq)
{
    if (n <= 0) return hipSuccess;
    best_particle_kernel<<<1, 1024, 0, stream>>>(v, n, px, py, pth, first_id, out5, h_out5, h_seq, seq);
    return hipGetLastError();
}

hipError_t launch_pose_sums(hipStream_t stream, const float* x, const float* y, const float* th, const int32_t* idx,
                            int n, float ref_th, unsigned long long* acc, unsigned int* ticket, long long* out,
                            long long* h_out, uint32_t* h_seq, uint32_t seq, const float* carry)
{
    if (n <= 0) return hipSuccess;
    const int nb = blocks_for(n) < 256 ? blocks_for(n) : 256;
    if (carry)
        pose_sums_kernel<true><<<nb, kBlock, 0, stream>>>(x, y, th, idx, carry, n, ref_th, acc, ticket, out, h_out, h_seq, seq);
    else
        pose_sums_kernel<false><<<nb, kBlock, 0, stream>>>(x, y, th, idx, nullptr, n, ref_th, acc, ticket, out, h_out, h_seq, seq);
    return hipGetLastError();
}

hipError_t launch_gather_f32(hipStream_t stream, const float* src, const int32_t* idx, int n, float* dst)
{
    if (n <= 0) return hipSuccess;
    gather_f32_kernel<<<blocks_for(n), kBlock, 0, stream>>>(src, idx, n, dst);
    return hipGetLastError();
}

hipError_t launch_gather_map(hipStream_t stream, const float* in, float* out, int64_t in_row_stride,
                             int64_t out_row_stride, int in_plane_stride, int out_plane_stride, int nlandmarks,
                             const int32_t* idx, int n)
{
    if (n <= 0 || nlandmarks <= 0) return hipSuccess;
    gather_map_kernel<<<n, kBlock, 0, stream>>>(in, out, in_row_stride, out_row_stride, in_plane_stride,
                                                out_plane_stride, nlandmarks, idx, n);
    return hipGetLastError();
}

}  // namespace slam
