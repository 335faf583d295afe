// scan_kernels.hip — the integer CDF of a frame's weights: the staged prefix sum over quantised weights, and the
// fused form that quantises and scans in one pass (with the ESS gate's sums, the shard's sums for several GPUs, and — on a frame
// whose front launch made the weights — the covariance classes' update behind its tiles).
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "block_reduce.h"
#include "cov_update_body.h"
#include "det_math.h"
#include "resample_common.h"

namespace slam {

namespace {

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

// ---- fused frame-loop form: weights are quantised and scanned in one pass, never stored.  The maximum: *d_max, or that of the
// block maxima, which every workgroup works out again (block_max_of).
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
    if (GATED) {   // (the scan has ended on a barrier: s_wave is free)
        const uint64_t a = block_sum_u64(s16, s_wave), b = block_sum_u64<false>(q16, s_wave);
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
// (cov_update_body.h), as logweight_cov_kernel (weights_kernels.hip) carries it: on a frame whose front launch has made the weights
// itself (frame_particle_kernel, front_kernels.hip) there is no weights' launch for it to ride in.
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

}  // namespace

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

}  // namespace slam
