// comb_quotient.h — the exact quotient of the offspring offsets where the offsets sit on a latency-bound chain
// (resample_kernels.hip: offspring_fill_kernel).  Plain C++ on purpose: tests/comb_quotient_driver.cpp walks it on the host.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
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

}  // namespace slam
