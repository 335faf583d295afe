// pf_common.h — what the particle-filter units (ekf_kernels.hip, front_kernels.hip, ekf_sparse_kernels.hip, paged_kernels.hip, split_kernels.hip, resample_kernels.hip, shard_kernels.hip) share.
#pragma once
#include "kernels.h"

namespace slam {
constexpr int kBlock = 256;   // threads per workgroup of every kernel that does not say otherwise
inline int blocks_for(int n) { return (n + kBlock - 1) / kBlock; }
inline int blocks256(int64_t n) { return (int)((n + 255) / 256); }   // ... for element counts beyond an int
}  // namespace slam
