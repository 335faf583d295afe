// comb_quotient.h — the comb of the systematic resample, written once for every kernel that lays it (resample_kernels.hip): the
// draw of its offset, the total no comb can be laid over, and first[] of a particle from its exclusive CDF — through long division,
// or through quotient_below_2_32 where the offsets sit on a latency-bound chain (offspring_fill_kernel).  quotient_below_2_32 is
// plain C++ on purpose: tests/comb_quotient_driver.cpp walks it on the host.  The rest is device code.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include "det_math.h"
#define SLAM_HOST_DEVICE __host__ __device__ __forceinline__
#else
#define SLAM_HOST_DEVICE inline
#endif

namespace slam {

// floor((hi:lo) / d) for 0 < d < 2^63 and a quotient below 2^32 (an offspring offset: at most the number of slots, < 2^31).
// A double-precision quotient proposes it — the conversions, the sum and the division each round once, a relative error below
// 2^-50, so the proposal is less than 2^-18 away from the real quotient and its floor at most one off —, and exact 128-bit integer
// comparisons settle it: q * d <= X < (q + 1) * d.  Two steps each way, twice what the bound asks for; no loop, no long division
// (div128by64 is a chain of 64 dependent steps).  Outside the precondition the result is some number, never a fault.
SLAM_HOST_DEVICE uint64_t quotient_below_2_32(uint64_t hi, uint64_t lo, uint64_t d)
{
    const double x = (double)hi * 18446744073709551616.0 + (double)lo;
    double qd = x / (double)d;
    qd = qd < 4294967295.0 ? qd : 4294967295.0;   // (also what a NaN from d = 0 becomes)
    qd = qd > 0.0 ? qd : 0.0;
    uint64_t q = (uint64_t)qd;
    const unsigned __int128 X = ((unsigned __int128)hi << 64) | lo;
    unsigned __int128 p = (unsigned __int128)q * d;
    if (p > X) { --q; p -= d; }
    if (p > X) { --q; p -= d; }
    if (X - p >= d) { ++q; p += d; }
    if (X - p >= d) { ++q; }
    return q;
}

#if defined(__HIPCC__)
// A total of 0 or >= 2^63 is impossible with finite log-weights (the best particle has wq = 2^32); stay memory-safe anyway: no
// draw, no division, first[] = 0 everywhere — every slot gets the last particle.
__device__ __forceinline__ bool comb_total_unusable(uint64_t total) { return total == 0 || (total >> 63); }

// comb offset u in [0, total): Philox counter (0, 0, frame, 1), high 64 bits of r64 * total (wave-uniform)
__device__ __forceinline__ uint64_t comb_draw(uint64_t total, uint32_t key0, uint32_t key1, uint32_t frame)
{
    const u32x4 r = philox4x32_10(0u, 0u, frame, 1u /* resample stream */, key0, key1);
    return __umul64hi((uint64_t)r.v[0] | ((uint64_t)r.v[1] << 32), total);
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

// first[] of a particle whose exclusive CDF is c_excl, with the offset drawn and the total usable: ceil((c_excl * n_total - u) /
// total) clamped at 0, as (X - u - 1) / total + 1 with X = c_excl * n_total in 128 bits.  kQuick: the quotient without the 64-step
// division (needs c_excl <= total, so that it is at most n_total < 2^31).
template <bool kQuick>
__device__ __forceinline__ int32_t comb_first_drawn(uint64_t c_excl, uint64_t total, uint64_t n_total, uint64_t comb_u)
{
    uint64_t lo = c_excl * n_total, hi = __umul64hi(c_excl, n_total);
    if (hi == 0 && lo <= comb_u) return 0;
    const uint64_t sub = comb_u + 1ull;   // comb_u < total < 2^63: no overflow
    hi -= lo < sub ? 1ull : 0ull;
    lo -= sub;
    return (int32_t)((kQuick ? quotient_below_2_32(hi, lo, total) : div128by64(hi, lo, total)) + 1ull);
}

// ... from the total alone: what the offsets kernels store (offspring_fill_kernel draws once for its two bounds and calls
// comb_first_quick)
__device__ __forceinline__ int32_t comb_first(uint64_t c_excl, uint64_t total, uint64_t n_total, uint32_t key0, uint32_t key1,
                                              uint32_t frame)
{
    if (comb_total_unusable(total)) return 0;
    return comb_first_drawn<false>(c_excl, total, n_total, comb_draw(total, key0, key1, frame));
}
__device__ __forceinline__ int32_t comb_first_quick(uint64_t c_excl, uint64_t total, uint64_t n_total, uint64_t comb_u)
{
    return comb_first_drawn<true>(c_excl, total, n_total, comb_u);
}
#endif

}  // namespace slam
