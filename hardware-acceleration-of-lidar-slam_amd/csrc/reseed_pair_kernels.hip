// reseed_pair_kernels.hip — reseeding the particle cloud from detection PAIRS (specification: tests/_reseed_pair_spec.py;
// DESIGN.md section 7, "Reseeding from detection pairs"): a chosen fraction of the slots is replaced by pose proposals at each of
// which TWO detections of the frame coincide with TWO landmarks of the known map — the heading is fixed, not drawn.  The first
// landmark and both detections are drawn; the second landmark is searched for among those that stand at the detections' distance
// from the first, by the wavefront: 64 lanes test 64 landmarks at a time for one chosen lane after another.  The other slots take
// the pending resample.  One launch; the four counts are exact integers, handed over by the last workgroup to arrive.
//
// No reference counterpart: the specification is DESIGN.md + tests/_reseed_pair_spec.py, matched bit for bit.

#include "det_math.h"
#include "pf_common.h"

namespace slam {

namespace {

// lane `owner`'s value in a scalar register (owner is wave-uniform: it comes from a ballot)
__device__ __forceinline__ int wave_read(int v, int owner) { return __builtin_amdgcn_readlane(v, owner); }
__device__ __forceinline__ float wave_read(float v, int owner) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), owner)); }

// is landmark j a partner of the landmark at (mx1, my1)?  squared distances only; both bounds inclusive
__device__ __forceinline__ bool pair_partner(const ReseedPairArgs& a, int j, int j1, float mx1, float my1, float lo2, float hi2)
{
    if (j >= a.nlandmarks || j == j1) return false;
    if (a.map[2 * (int64_t)a.plane_stride + j] < 0.0f) return false;
    const float bx = a.map[j] - mx1, by = a.map[a.plane_stride + j] - my1;
    const float t = bx * bx;
    const float u = by * by;
    const float dm2 = t + u;
    return dm2 > 0.0f && lo2 <= dm2 && dm2 <= hi2;
}

// Slot i, gid = first_id + i: rA = Philox(gid, frame, stream 2), the stream and the threshold of pose_reseed_kernel, so the same
// slots are chosen.  j1 = umulhi(rA1, L), k1 = umulhi(rA2, K), k2 = umulhi(rA3, K - 1) stepped over k1.  a = z_k2 - z_k1 shorter
// than min_sep (or not a number): flag 3; slot j1 empty: flag 2; else the wavefront counts the partners of j1, picks the
// umulhi(rB0, cnt)-th in landmark order (rB: stream 3; none: flag 4), and the owning lane makes the pose: heading
// atan2(b x a, a . b) with b = m_j2 - m_j1, position as pose_reseed_kernel's.  Every product, sum, quotient and root rounded on its
// own (-ffp-contract=off), in the order of the specification.  Slots that are not replaced copy the pose of anc[i] (nullptr: i);
// in place (out == in) is sound exactly then.  No lane leaves before the wave's loop: ballots and lane reads need all 64.
__global__ __launch_bounds__(kBlock) void pose_reseed_pairs_kernel(const ReseedPairArgs a)
{
    __shared__ uint32_t s_cnt[4][kBlock / 64];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    int flag = 0;
    bool search = false;
    uint32_t j1 = 0, k1 = 0;
    uint64_t gid = 0;
    float ax = 0.0f, ay = 0.0f, mx1 = 0.0f, my1 = 0.0f, lo2 = 0.0f, hi2 = 0.0f;
    if (i < a.n) {
        gid = a.first_id + (uint64_t)i;
        const u32x4 r = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), a.frame, 2u /* reseed stream */, a.key0, a.key1);
        if ((uint64_t)r.v[0] < a.thr) {
            j1 = __umulhi(r.v[1], (uint32_t)a.nlandmarks);   // < nlandmarks <= plane_stride
            k1 = __umulhi(r.v[2], (uint32_t)a.ndet);         // < ndet
            uint32_t k2 = __umulhi(r.v[3], (uint32_t)a.ndet - 1u);
            k2 += k2 >= k1;                                  // < ndet, != k1
            ax = a.det_zx[k2] - a.det_zx[k1];
            ay = a.det_zy[k2] - a.det_zy[k1];
            const float t = ax * ax;
            const float u = ay * ay;
            const float dz2 = t + u;
            if (!(dz2 >= a.min_sep2)) flag = 3;              // (NaN: too close)
            else if (a.map[2 * (int64_t)a.plane_stride + j1] < 0.0f) flag = 2;
            else {
                search = true;
                const float dz = sqrtf(dz2);                 // sqrtf: correctly rounded (NOT __fsqrt_rn)
                const float lo = dz - a.tol, hi = dz + a.tol;
                lo2 = lo * lo;
                hi2 = hi * hi;
                mx1 = a.map[j1];
                my1 = a.map[a.plane_stride + j1];
            }
        }
    }
    // the wavefront serves its searching lanes one after another, lowest first; everything below the loop head is wave-uniform
    int j2 = -1;
    const int chunks = (a.nlandmarks + 63) >> 6;
    for (unsigned long long todo = __ballot(search); todo; todo &= todo - 1) {
        const int owner = __ffsll(todo) - 1;
        const int oj1 = wave_read((int)j1, owner);
        const float omx = wave_read(mx1, owner), omy = wave_read(my1, owner), olo2 = wave_read(lo2, owner), ohi2 = wave_read(hi2, owner);
        uint32_t cnt = 0;
        for (int q = 0; q < chunks; ++q)
            cnt += (uint32_t)__popcll(__ballot(pair_partner(a, 64 * q + lane, oj1, omx, omy, olo2, ohi2)));
        int found = -1;
        if (cnt) {
            uint32_t c = 0;
            if (lane == owner) {
                const u32x4 rb = philox4x32_10((uint32_t)gid, (uint32_t)(gid >> 32), a.frame, 3u /* partner stream */, a.key0, a.key1);
                c = __umulhi(rb.v[0], cnt);                  // < cnt
            }
            c = (uint32_t)wave_read((int)c, owner);
            for (int q = 0; q < chunks; ++q) {               // to the chunk that holds the c-th partner
                const unsigned long long m = __ballot(pair_partner(a, 64 * q + lane, oj1, omx, omy, olo2, ohi2));
                const uint32_t pc = (uint32_t)__popcll(m);
                if (c < pc) {                                // the lane of rank c within the chunk's ballot
                    const bool mine = ((m >> lane) & 1ull) && (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) == c;
                    found = 64 * q + (__ffsll(__ballot(mine)) - 1);
                    break;
                }
                c -= pc;
            }
        }
        if (lane == owner) j2 = found;
    }
    bool replaced = false;
    if (i < a.n) {
        float x, y, th;
        if (search && j2 < 0) flag = 4;
        if (search && j2 >= 0) {
            replaced = true;
            flag = 1;
            const float bx = a.map[j2] - mx1, by = a.map[a.plane_stride + j2] - my1;
            float t = bx * ay;
            float u = by * ax;
            const float cr = t - u;
            t = ax * bx;
            u = ay * by;
            const float dt = t + u;
            th = det_atan2f(cr, dt);
            if (th < 0.0f) th = th + 6.2831853072f;
            float s, c;
            det_sincosf(th, s, c);
            const float zx = a.det_zx[k1], zy = a.det_zy[k1];
            t = c * zx;
            float v = s * zy;
            t = t + v;
            x = mx1 - t;
            t = c * zy;
            v = s * zx;
            t = t - v;
            y = my1 - t;
        } else {
            const int64_t src = a.anc ? (int64_t)a.anc[i] : i;
            x = a.x_in[src];
            y = a.y_in[src];
            th = a.th_in[src];
        }
        a.x_out[i] = x;
        a.y_out[i] = y;
        a.th_out[i] = th;
        if (a.flag) a.flag[i] = (uint8_t)flag;
    }
    // the workgroup's four counts, then one atomic each; the last workgroup to arrive hands the totals over — to device memory and,
    // optionally, mapped host memory behind a sequence number — and clears the accumulators and the ticket for the next call
    const uint32_t c0 = (uint32_t)__popcll(__ballot(replaced)), c1 = (uint32_t)__popcll(__ballot(flag == 2)),
                   c2 = (uint32_t)__popcll(__ballot(flag == 3)), c3 = (uint32_t)__popcll(__ballot(flag == 4));
    if (lane == 0) {
        s_cnt[0][threadIdx.x >> 6] = c0;
        s_cnt[1][threadIdx.x >> 6] = c1;
        s_cnt[2][threadIdx.x >> 6] = c2;
        s_cnt[3][threadIdx.x >> 6] = c3;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    uint32_t sum[4] = { 0, 0, 0, 0 };
    for (int w = 0; w < kBlock / 64; ++w)
        for (int k = 0; k < 4; ++k) sum[k] += s_cnt[k][w];
    unsigned int* ticket = a.acc + 4;
    for (int k = 0; k < 4; ++k)
        if (sum[k]) atomicAdd(&a.acc[k], sum[k]);
    __threadfence();
    if (atomicAdd(ticket, 1u) != gridDim.x - 1) return;
    __threadfence();
    int32_t r[4];
    for (int k = 0; k < 4; ++k) r[k] = (int32_t)atomicExch(&a.acc[k], 0u);
    *ticket = 0;
    for (int k = 0; k < 4; ++k) a.out[k] = r[k];
    if (a.h_out) {
        for (int k = 0; k < 4; ++k) a.h_out[k] = r[k];
        __threadfence_system();
        __hip_atomic_store(a.h_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_pose_reseed_pairs(hipStream_t stream, const ReseedPairArgs& a, const EventPair* ev)
{
    if (a.n <= 0 || a.ndet < 2 || a.nlandmarks < 2) return hipSuccess;
    if (ev) (void)hipEventRecord(ev->start, stream);
    pose_reseed_pairs_kernel<<<blocks256(a.n), kBlock, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
