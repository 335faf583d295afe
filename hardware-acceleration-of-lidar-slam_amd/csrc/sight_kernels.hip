// sight_kernels.hip — the sight table behind the line of sight of the existence evidence (no counterpart in the reference;
// specification: tests/_sight_spec.py): a landmark that lies BEHIND what the frame's scan hit in its direction
// is hidden and takes no miss, so a pole that passes behind another pole or a wall keeps its slot, its mean and its covariance.
// The stage that reads the table: evidence_stage_kernel with SIGHT (evidence_kernels.hip).
//
// Directions are `bins` (a power of two, 32 .. 1024) equal steps of the DIAMOND ANGLE p in [0, 4) of a sensor-frame point: with
// q = |y| / (|x| + |y|), p = q, 2 - q, 2 + q, 4 - q by quadrant — monotone in the true angle, one IEEE division, no arctangent.
// sight_table_kernel: ONE WORKGROUP, one launch over the engine's current scan (a latency kernel like the detector): an LDS table
// of `bins` words starts as +inf; every point takes the unsigned minimum of its bin with the bits of r2 = x*x + y*y (non-negative
// floats order as their bits, and a minimum does not depend on the order of arrival); one coalesced store of kSightMaxBins floats
// (+inf from `bins` on) to the engine's buffer.

#include "evidence_common.h"

namespace slam {

namespace {

constexpr unsigned kInfBits = 0x7f800000u;

// the bin of the sensor-frame point (x, y): false — none (the origin, a point that is not finite): its diamond angle, binned
// (evidence_common.h)
__device__ __forceinline__ bool sight_bin(float x, float y, float quarter, unsigned mask, unsigned& j)
{
    float p;
    const bool has = diamond_angle(x, y, p);
    j = diamond_bin(p, quarter, mask);
    return has;
}

__global__ __launch_bounds__(1024) void sight_table_kernel(const float* bx, const float* by, int nbeams, int bins, float* out)
{
    __shared__ unsigned s_tab[kSightMaxBins];
    const int T = (int)blockDim.x, tid = (int)threadIdx.x;
    for (int j = tid; j < kSightMaxBins; j += T) s_tab[j] = kInfBits;
    __syncthreads();
    const float quarter = (float)(bins >> 2);
    const unsigned mask = (unsigned)bins - 1u;
    for (int b = tid; b < nbeams; b += T) {
        const float x = bx[b], y = by[b];
        unsigned j;
        if (sight_bin(x, y, quarter, mask, j)) {
            const float xx = x * x, yy = y * y;
            atomicMin(&s_tab[j], __float_as_uint(xx + yy));   // ds_min_u32: x and y are finite here, the sum is >= 0 or +inf
        }
    }
    __syncthreads();
    for (int j = tid; j < kSightMaxBins; j += T) out[j] = __uint_as_float(s_tab[j]);
}

}  // namespace

bool sight_bins_ok(int bins) { return bins >= kSightMinBins && bins <= kSightMaxBins && (bins & (bins - 1)) == 0; }

hipError_t launch_sight_table(hipStream_t stream, const float* bx, const float* by, int nbeams, int bins, float* out, const EventPair* ev)
{
    if (nbeams < 0 || nbeams > SLAM_MAX_BEAMS || !sight_bins_ok(bins) || !out || (nbeams > 0 && (!bx || !by))) return hipErrorInvalidValue;
    int threads = (nbeams + 63) & ~63;
    threads = threads < 64 ? 64 : threads > 1024 ? 1024 : threads;
    if (ev) (void)hipEventRecord(ev->start, stream);
    sight_table_kernel<<<1, threads, 0, stream>>>(bx, by, nbeams, bins, out);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
