// pf_common.h — what the particle-filter units (ekf_kernels.hip, front_kernels.hip, ekf_sparse_kernels.hip, paged_kernels.hip, split_kernels.hip, weights_kernels.hip, scan_kernels.hip, resample_kernels.hip, estimate_kernels.hip, shard_kernels.hip) share.
// (The workgroup-wide reductions and the scan: block_reduce.h.)
#pragma once
#include "kernels.h"

namespace slam {
constexpr int kBlock = 256;   // threads per workgroup of every kernel that does not say otherwise
inline int blocks_for(int n) { return (n + kBlock - 1) / kBlock; }

// ---- the weights of a frame, shared by the launches that make them (weights_kernels.hip: logweight_kernel,
// logweight_cov_kernel; front_kernels.hip: frame_particle_kernel)
// a particle's log-weight from its log-likelihood and its score times the gain.  carry (optional): the normalised log-weights the
// previous frame left behind; they count only when that frame did NOT resample (add_carry)
__device__ __forceinline__ float log_weight_of(float ll, float sc, const float* __restrict__ carry, bool add_carry, int i)
{
    float lw = ll - sc;
    if (add_carry) lw = carry[i] + lw;
    return lw;
}
__device__ __forceinline__ float wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
inline int blocks256(int64_t n) { return (int)((n + 255) / 256); }   // ... for element counts beyond an int
}  // namespace slam
