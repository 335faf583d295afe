// block_reduce.h — the workgroup-wide steps of the weights, scan, resample, estimate and shard units, each written once: the sum of a
// u64, the maximum of a float, the inclusive scan of one value per thread.  All are for workgroups of kBlock threads and take kBlock / 64
// words of LDS from the caller.
// kFree (default): the step ends on a barrier, so the caller may write the scratch again at once.  kFree = false is for the scratch's
// last use: one barrier less, and nothing may write the scratch before the workgroup's next barrier.
#pragma once
#include "pf_common.h"

namespace slam {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        v += ((uint64_t)hi << 32) | lo;
    }
    return v;
}

// the sum in every thread (integers: exact, whatever the order)
template <bool kFree = true>
__device__ __forceinline__ uint64_t block_sum_u64(uint64_t v, uint64_t* s_red /*[kBlock/64]*/)
{
    v = wave_sum_u64(v);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t r = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) r += s_red[w];
    if (kFree) __syncthreads();
    return r;
}

// the maximum in every thread.  The wavefronts' maxima are folded with fmaxf from s_red[0] on, in wavefront order — in thread 0,
// s_red[0] is the thread's own wave_max.  (What goes in is a running maximum kept with `>`, so no NaN arrives here.)
template <bool kFree = true>
__device__ __forceinline__ float block_max(float m, float* s_red /*[kBlock/64]*/)
{
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = m;
    __syncthreads();
    float r = s_red[0];
#pragma unroll
    for (int w = 1; w < kBlock / 64; ++w) r = fmaxf(r, s_red[w]);
    if (kFree) __syncthreads();
    return r;
}

// ... of an array of block maxima, read by the whole workgroup (<= 2048 floats).  The same steps as block_max, written out and not
// called: through the call the compiler orders two instructions of the frame path's scan (quantise_scan_body) differently, and that
// kernel keeps its instruction stream.
template <bool kFree = true>
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
    if (kFree) __syncthreads();
    return r;
}

__device__ __forceinline__ uint64_t shfl_up(uint64_t v, int d)
{
    const uint32_t lo = __shfl_up((uint32_t)v, d), hi = __shfl_up((uint32_t)(v >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ int32_t shfl_up(int32_t v, int d) { return __shfl_up(v, d); }

// inclusive scan of one value per thread over the workgroup: wavefront scan + carry through LDS; total: the sum over the workgroup
template <class T, bool kFree = true>
__device__ __forceinline__ T block_inclusive_scan(T v, T* s_wave /*[kBlock/64]*/, T& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const T up = shfl_up(v, d);
        if (lane >= d) v += up;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    T carry = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) carry += s_wave[w];
        tot += s_wave[w];
    }
    total = tot;
    if (kFree) __syncthreads();
    return v + carry;
}

}  // namespace slam
