// resample_common.h — what the units of the integer resample (scan_kernels.hip, resample_kernels.hip, shard_kernels.hip) must agree on:
// the tile of the scan and the search over first[].
#pragma once
#include "pf_common.h"

namespace slam {

constexpr int kScanItems = 8;                       // elements per thread
constexpr int kScanTile = kBlock * kScanItems;      // 2048 elements per workgroup: the tile of cdf_local / tile_total

// the ancestor of slot j: the last particle whose first slot (first_all, non-decreasing) is <= j
__device__ __forceinline__ int64_t last_with_first_le(const int32_t* __restrict__ first_all, int64_t n_total, int64_t j)
{
    int64_t lo = 0, hi = n_total;   // first index whose first slot is > j
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)first_all[mid] <= j) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

}  // namespace slam
