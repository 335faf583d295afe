// weights_kernels.hip — the weights of a frame: log-weights (with the covariance classes' update riding along)
// and their block maxima, the maximum as one float, the staged quantisation.  (On a frame whose front launch made the weights —
// front_kernels.hip: frame_particle_kernel — none of this runs; the classes' update rides behind the scan's tiles instead.)
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "block_reduce.h"
#include "cov_update_body.h"
#include "det_math.h"

namespace slam {

namespace {

// (log_weight_of, wave_max: pf_common.h)
// The log-weights of the particles block, block + nblocks, .. (in units of kBlock) and their maximum, by one workgroup
// (logweight_kernel: the whole grid; logweight_cov_kernel: its first part).
// carry (optional): the normalised log-weights the previous frame left behind; they count only when that frame did
// NOT resample (*prev_resampled == 0, a device flag written by the previous frame's resample kernel)
__device__ __forceinline__ void logweight_body(const float* __restrict__ score, const float* __restrict__ loglik, float gain, int n,
                                               const float* __restrict__ carry, const int32_t* __restrict__ prev_resampled,
                                               float* __restrict__ logw, float* __restrict__ block_max_out, int block, int nblocks)
{
    __shared__ float s_max[kBlock / 64];
    float m = -INFINITY;
    const bool add_carry = carry && *prev_resampled == 0;
    for (int i = block * kBlock + threadIdx.x; i < n; i += nblocks * kBlock) {
        const float ll = loglik ? loglik[i] : 0.0f;
        const float sc = score ? score[i] * gain : 0.0f;
        const float lw = log_weight_of(ll, sc, carry, add_carry, i);
        logw[i] = lw;
        m = lw > m ? lw : m;   // NaN never enters, the first of two equal zeros stays
    }
    m = block_max<false>(m, s_max);
    if (threadIdx.x == 0) block_max_out[block] = m;
}

__global__ __launch_bounds__(kBlock) void logweight_kernel(const float* __restrict__ score,
                                                           const float* __restrict__ loglik, float gain, int n,
                                                           const float* __restrict__ carry,
                                                           const int32_t* __restrict__ prev_resampled,
                                                           float* __restrict__ logw, float* __restrict__ block_max)
{
    logweight_body(score, loglik, gain, n, carry, prev_resampled, logw, block_max, blockIdx.x, gridDim.x);
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
    logweight_body(score, loglik, gain, n, carry, prev_resampled, logw, block_max, blockIdx.x, nw);
}

// Several GPUs: the maximum of the block maxima as one float for the all-reduce.  (Folding this into the kernel above with
// a "last workgroup done" ticket was measured and dropped: two atomics per workgroup on one address run at ~88 per
// microsecond, 47 us at 2048 workgroups against 5 us for this launch.)
__global__ __launch_bounds__(kBlock) void max_finalize_kernel(const float* __restrict__ block_max, int nblocks,
                                                              float* __restrict__ d_max)
{
    __shared__ float s_max[kBlock / 64];
    const float m = block_max_of<false>(block_max, nblocks, s_max);
    if (threadIdx.x == 0) *d_max = m;
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
    acc = block_sum_u64<false>(acc, s_sum);
    if (threadIdx.x == 0) atomicAdd(d_sum, (unsigned long long)acc);   // integer: exact and order-independent
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

}  // namespace slam
