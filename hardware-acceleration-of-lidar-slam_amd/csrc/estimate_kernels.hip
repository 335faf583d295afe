// estimate_kernels.hip — what is read out of a population: the heaviest particle (arg-max, or with its pose in one launch), the
// exact sums for the posterior mean and for the second moments about it, and the gathers through the resample indices (gather_f32, gather_map).
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "block_reduce.h"
#include "det_math.h"

namespace slam {

namespace {

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

// The largest of v[0..n) and its index, by ONE workgroup of kBestBlock threads: the lowest index on ties, NaN never wins, and
// with nothing but -inf and NaN the index is 0 (the value is then -inf).  The result is thread 0's.
constexpr int kBestBlock = 1024;
struct Best {
    float v;
    int i;
    __device__ __forceinline__ void take(float ov, int oi)
    {
        if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
    }
};
__device__ __forceinline__ Best block_argmax(const float* __restrict__ v, int n)
{
    __shared__ float s_v[kBestBlock / 64];
    __shared__ int s_i[kBestBlock / 64];
    Best b = { -INFINITY, 0x7fffffff };
    for (int i = threadIdx.x; i < n; i += kBestBlock) b.take(v[i], i);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) b.take(__shfl_xor(b.v, o), __shfl_xor(b.i, o));
    if ((threadIdx.x & 63) == 0) { s_v[threadIdx.x >> 6] = b.v; s_i[threadIdx.x >> 6] = b.i; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBestBlock / 64; ++w) b.take(s_v[w], s_i[w]);
        if (!(b.v > -INFINITY)) b.i = 0;
    }
    return b;
}

// index of the largest value (the heaviest particle); one workgroup
__global__ __launch_bounds__(kBestBlock) void argmax_kernel(const float* __restrict__ v, int n, int32_t* __restrict__ idx_out,
                                                            float* __restrict__ val_out)
{
    const Best b = block_argmax(v, n);
    if (threadIdx.x == 0) {
        *idx_out = b.i;
        *val_out = b.v;
    }
}

// The heaviest particle with its pose, in one launch: {logw, global id, x, y, theta} to device memory and, optionally,
// to mapped host memory behind a sequence number (a plain C host then needs no copy and no stream synchronisation).
__global__ __launch_bounds__(kBestBlock) void best_particle_kernel(const float* __restrict__ v, int n,
                                                                   const float* __restrict__ px, const float* __restrict__ py,
                                                                   const float* __restrict__ pth, int64_t first_id,
                                                                   float* __restrict__ out5, float* __restrict__ h_out5,
                                                                   uint32_t* __restrict__ h_seq, uint32_t seq)
{
    const Best b = block_argmax(v, n);
    if (threadIdx.x != 0) return;
    const float r[5] = { b.v, __int_as_float((int32_t)(first_id + b.i)), px[b.i], py[b.i], pth[b.i] };
    for (int k = 0; k < 5; ++k) out5[k] = r[k];
    if (h_out5) {
        for (int k = 0; k < 5; ++k) h_out5[k] = r[k];
        __threadfence_system();
        __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// The end of the kernels that sum over the population: the workgroup's sums into the accumulators, one atomic each; the last
// workgroup to finish (a ticket) hands the totals over — to device memory and, optionally, mapped host memory behind a sequence
// number — and clears the accumulators and the ticket for the next call.
template <int kSums>
__device__ __forceinline__ void hand_over_sums(uint64_t (&sum)[kSums], unsigned long long* __restrict__ acc,
                                               unsigned int* __restrict__ ticket, long long* __restrict__ out,
                                               long long* __restrict__ h_out, uint32_t* __restrict__ h_seq, uint32_t seq)
{
    __shared__ uint64_t s_red[kBlock / 64];
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

// Exact, order-independent sums over the population for the posterior mean: x and y as 2^-32 fixed point, the heading
// as sin / cos of (theta - ref) in 2^-30 fixed point (det_sincosf: the specified polynomial), accumulated with 64-bit
// integer atomics — the same bits for any summation order, workgroup count or sharding.  idx (optional): the pending
// resample gather.  The sums are handed over by hand_over_sums.
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
    hand_over_sums<kSums>(sum, acc, ticket, out, h_out, h_seq, seq);
}

// Exact, order-independent second moments of the population about the mean the sums above gave (slam_pf_spread; DESIGN.md
// section 7): per particle dx = x - mean_x, dy = y - mean_y (one binary32 subtraction each) and s = the sine det_sincosf gives for
// theta - mean_theta, cast to 2^-20 fixed point towards zero: DX, DY, SS.  Six sums of w * A * B and D = sum w, with w = 1 or
// (WEIGHTED) the w16 of pose_sums_kernel; same block size, ticket and hand-over.
// Limbs: |dx|, |dy| < 2048 m makes |DX|, |DY| < 2^31 (|SS| <= 2^20), so a product P = A * B is ONE 32 x 32 -> 64-bit signed
// multiply, |P| < 2^62.  P goes in as three limbs, P & 0x1fffff, (P >> 21) & 0x1fffff (both in [0, 2^21)) and P >> 42 (arithmetic:
// |P >> 42| <= 2^20), each times w <= 2^16 — again one 32 x 32 -> 64-bit multiply-add.  A limb term is below 2^37 in size and
// n_total <= 2^23 of them stay below 2^60 < 2^63, over all workgroups and all ranks; the host joins the limbs in 128 bits.
// A particle outside the domain (or with a NaN delta) counts in the flag word and adds zeros.
template <bool WEIGHTED>
__global__ __launch_bounds__(kBlock) void pose_moments_kernel(const float* __restrict__ x, const float* __restrict__ y,
                                                              const float* __restrict__ th, const int32_t* __restrict__ idx,
                                                              const float* __restrict__ carry, int n, float mean_x, float mean_y,
                                                              float mean_th, unsigned long long* __restrict__ acc,
                                                              unsigned int* __restrict__ ticket, long long* __restrict__ out,
                                                              long long* __restrict__ h_out, uint32_t* __restrict__ h_seq,
                                                              uint32_t seq)
{
    uint64_t sum[kPoseMoments];   // two's complement: signed sums through unsigned adds
#pragma unroll
    for (int k = 0; k < kPoseMoments; ++k) sum[k] = 0;
    for (int i = blockIdx.x * kBlock + threadIdx.x; i < n; i += gridDim.x * kBlock) {
        const int j = idx ? idx[i] : i;
        const float dx = x[j] - mean_x, dy = y[j] - mean_y;
        float s, c;
        det_sincosf(th[j] - mean_th, s, c);
        const bool inside = fabsf(dx) < 2048.0f && fabsf(dy) < 2048.0f;   // (false for NaN)
        const int32_t d[3] = { inside ? (int32_t)(dx * 1048576.0f) : 0, inside ? (int32_t)(dy * 1048576.0f) : 0,
                               (int32_t)(s * 1048576.0f) };
        const uint32_t w = WEIGHTED ? (uint32_t)((uint64_t)(det_expf(carry[i]) * 4294967296.0f) >> 16) : 1u;
        constexpr int kA[6] = { 0, 0, 1, 0, 1, 2 }, kB[6] = { 0, 1, 1, 2, 2, 2 };
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            const long long p = (long long)d[kA[k]] * (long long)d[kB[k]];
            const uint32_t p0 = (uint32_t)p & 0x1fffffu, p1 = (uint32_t)(p >> 21) & 0x1fffffu;
            const int32_t p2 = (int32_t)(p >> 42);
            sum[3 * k] += (uint64_t)w * p0;
            sum[3 * k + 1] += (uint64_t)w * p1;
            sum[3 * k + 2] += (uint64_t)((long long)(int32_t)w * (long long)p2);
        }
        sum[kPoseMomentsD] += w;
        sum[kPoseMomentsFlag] += inside ? 0u : 1u;
    }
    hand_over_sums<kPoseMoments>(sum, acc, ticket, out, h_out, h_seq, seq);
}

}  // namespace

hipError_t launch_argmax(hipStream_t stream, const float* v, int n, int32_t* idx_out, float* val_out)
{
    if (n <= 0) return hipSuccess;
    argmax_kernel<<<1, kBestBlock, 0, stream>>>(v, n, idx_out, val_out);
    return hipGetLastError();
}

hipError_t launch_best_particle(hipStream_t stream, const float* v, int n, const float* px, const float* py,
                                const float* pth, int64_t first_id, float* out5, float* h_out5, uint32_t* h_seq,
                                uint32_t seq)
{
    if (n <= 0) return hipSuccess;
    best_particle_kernel<<<1, kBestBlock, 0, stream>>>(v, n, px, py, pth, first_id, out5, h_out5, h_seq, seq);
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

hipError_t launch_pose_moments(hipStream_t stream, const float* x, const float* y, const float* th, const int32_t* idx,
                               int n, const float mean[3], unsigned long long* acc, unsigned int* ticket, long long* out,
                               long long* h_out, uint32_t* h_seq, uint32_t seq, const float* carry)
{
    if (n <= 0) return hipSuccess;
    // Eight particles per thread, at most 64 workgroups: every workgroup ends on 20 atomics to the same 20 words, and that fixed part,
    // not the bytes, bounds the launch (profiles/spread.md: 256 workgroups took 55 us here at 65 536 particles, 32 take 23 us)
    const int want = (blocks_for(n) + 7) / 8;
    const int nb = want < 1 ? 1 : want < 64 ? want : 64;
    if (carry)
        pose_moments_kernel<true><<<nb, kBlock, 0, stream>>>(x, y, th, idx, carry, n, mean[0], mean[1], mean[2], acc, ticket, out, h_out, h_seq, seq);
    else
        pose_moments_kernel<false><<<nb, kBlock, 0, stream>>>(x, y, th, idx, nullptr, n, mean[0], mean[1], mean[2], acc, ticket, out, h_out, h_seq, seq);
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
