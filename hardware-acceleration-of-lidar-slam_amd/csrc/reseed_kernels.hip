// reseed_kernels.hip — reseeding the particle cloud from what the lidar sees (specification: tests/_reseed_spec.py; DESIGN.md
// section 7, "Reseeding in a known map"): a chosen fraction of the slots is replaced by pose proposals at each of which one
// detection of the frame coincides with one landmark of the known map; the other slots take the pending resample.  One thread per
// slot, one launch; the two counts are exact integers, handed over by the last workgroup to arrive.
//
// No reference counterpart: the specification is DESIGN.md + tests/_reseed_spec.py, matched bit for bit.

#include "det_math.h"
#include "pf_common.h"

namespace slam {

namespace {

// Slot i, gid = first_id + i: r = Philox(gid, frame, stream 2).  Chosen iff r0 < thr; landmark j = umulhi(r1, L), detection
// k = umulhi(r2, K), heading theta = 2 pi * (r3 >> 8) * 2^-24; the position is the update's w = p + H^T z read backwards, every
// product and sum rounded on its own (-ffp-contract=off) in the order of the specification.  A chosen slot whose landmark slot is
// empty (P_xx < 0) is not replaced.  Slots that are not replaced copy the pose of anc[i] (nullptr: i) — in place (out == in) is
// sound exactly then: every thread reads and writes its own slot only.
__global__ __launch_bounds__(kBlock) void pose_reseed_kernel(const ReseedArgs a)
{
    __shared__ uint32_t s_cnt[2][kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool replaced = false, empty = false;
    if (i < a.n) {
        const uint64_t gid = a.first_id + (uint64_t)i;
        const u32x4 r = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), a.frame, 2u /* reseed stream */, a.key0, a.key1);
        float x = 0.0f, y = 0.0f, th = 0.0f;
        if ((uint64_t)r.v[0] < a.thr) {
            const uint32_t j = __umulhi(r.v[1], (uint32_t)a.nlandmarks);   // < nlandmarks <= plane_stride
            replaced = !(a.map[2 * (int64_t)a.plane_stride + j] < 0.0f);
            empty = !replaced;
            if (replaced) {
                const uint32_t k = __umulhi(r.v[2], (uint32_t)a.ndet);     // < ndet
                const float zx = a.det_zx[k], zy = a.det_zy[k];
                th = 6.2831853072f * ((float)(r.v[3] >> 8) * 5.9604644775390625e-8f);
                float s, c;
                det_sincosf(th, s, c);
                float t = c * zx;
                float v = s * zy;
                t = t + v;
                x = a.map[j] - t;
                t = c * zy;
                v = s * zx;
                t = t - v;
                y = a.map[a.plane_stride + j] - t;
            }
        }
        if (!replaced) {
            const int64_t src = a.anc ? (int64_t)a.anc[i] : i;
            x = a.x_in[src];
            y = a.y_in[src];
            th = a.th_in[src];
        }
        a.x_out[i] = x;
        a.y_out[i] = y;
        a.th_out[i] = th;
        if (a.flag) a.flag[i] = replaced ? 1 : empty ? 2 : 0;
    }
    // the workgroup's two counts, then one atomic each; the last workgroup to arrive hands the totals over — to device memory and,
    // optionally, mapped host memory behind a sequence number — and clears the accumulators and the ticket for the next call
    const uint32_t c0 = (uint32_t)__popcll(__ballot(replaced)), c1 = (uint32_t)__popcll(__ballot(empty));
    if ((threadIdx.x & 63) == 0) {
        s_cnt[0][threadIdx.x >> 6] = c0;
        s_cnt[1][threadIdx.x >> 6] = c1;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t sum[2] = { 0, 0 };
    for (int w = 0; w < kBlock / 64; ++w) {
        sum[0] += s_cnt[0][w];
        sum[1] += s_cnt[1][w];
    }
    unsigned int* ticket = a.acc + 2;
    if (sum[0]) atomicAdd(&a.acc[0], sum[0]);
    if (sum[1]) atomicAdd(&a.acc[1], sum[1]);
    __threadfence();
    if (atomicAdd(ticket, 1u) != gridDim.x - 1) return;
    __threadfence();
    const int32_t r0 = (int32_t)atomicExch(&a.acc[0], 0u), r1 = (int32_t)atomicExch(&a.acc[1], 0u);
    *ticket = 0;
    a.out[0] = r0;
    a.out[1] = r1;
    if (a.h_out) {
        a.h_out[0] = r0;
        a.h_out[1] = r1;
        __threadfence_system();
        __hip_atomic_store(a.h_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_pose_reseed(hipStream_t stream, const ReseedArgs& a, const EventPair* ev)
{
    if (a.n <= 0 || a.ndet <= 0) return hipSuccess;
    if (ev) (void)hipEventRecord(ev->start, stream);
    pose_reseed_kernel<<<blocks256(a.n), kBlock, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
