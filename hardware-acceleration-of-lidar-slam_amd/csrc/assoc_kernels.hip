// assoc_kernels.hip — data association (no counterpart in the reference; specification: tests/_assoc_spec.py, DESIGN.md
// section 7): the detections of a frame are sensor-frame points without identity, and every particle decides for itself which of
// its landmarks each one belongs to and which ones start a new landmark (associate_kernel); the landmark update then reads its
// observations through the particle's table (ekf_update_kernel of ekf_kernels.hip with EkfObsTable as its source of z).
// Rows only: a table per particle means "which landmarks a frame observes" differs between particles, which the split, paged
// and grouped forms rely on being the same.
//
// associate_kernel: ONE WAVEFRONT OWNS ONE PARTICLE, lanes own landmarks l and l + 64 of each batch of 128 (the access shape of
// ekf_row_body.h) and walk the K detections in a wave-uniform loop: (P + q I)^-1 once per landmark, then per detection the
// Mahalanobis term of the update's own likelihood on v2f (the operations of ekf_shared_from / ekf_particle, the same bits).
//   c. every landmark keeps its cheapest detection (strict <, k ascending: the lowest k on ties, NaN never wins);
//   d. the candidates (0 <= m <= gate) post (bits(m) << 32 | l) to an LDS 64-bit minimum per detection — m >= 0, so the
//      order of the bits is the order of the values, -0 is made +0 first, and l in the low word breaks ties towards the lowest
//      landmark: the result does not depend on the order in which lanes or batches arrive;
//   e. a detection that matched nothing and lies within new_gate of no seen landmark (a flag per detection, from a ballot, kept by lane k)
//      takes the next unseen slot: the ranks come from popcounts over a 64-bit "unseen" mask per 64 landmarks.
// The particle's table row is assembled in LDS and written out as whole dwords.
//
// Under a full 2x2 sensor-frame measurement covariance Q (specification: tests/_assoc_aniso_spec.py) association and update run
// with S = P + R_w(theta_i): associate_body takes the noise as a policy (AssocNoiseIso: the lines above; AssocNoiseAniso: R_w once
// per wavefront, S^-1 with the operations of ekf_aniso_update_one), and the update's noise policy is EkfNoiseAniso.
//
// Under a covariance PER DETECTION (specification: tests/_assoc_detcov_spec.py) S = P + R_w(theta_i, k) differs from detection
// to detection: AssocNoiseDet has lane k form R_w(theta_i, k) once (all K in one pass, beside the world-frame point it already
// holds), the loop over k reads it into scalar registers with the point, and S^-1 — the same operations, the same reciprocal —
// moves INSIDE that loop, per (landmark, detection) pair.  The update's noise policy is EkfNoiseDet.

#include "assoc_noise.h"

namespace slam {

namespace {

typedef unsigned long long u64;

// LDS of one wavefront, carved out of the dynamic region in multiples of 16 bytes:
//   best[64] u64 | unseen[2 * batches] u64 | fresh[64] u8 | row[nlandmarks rounded up to 16] u8
struct AssocLds {
    unsigned batches, rowb, per_wave;
};
__host__ __device__ inline AssocLds assoc_lds(unsigned L)
{
    AssocLds s;
    s.batches = (L + 127u) / 128u;
    s.rowb = (L + 15u) & ~15u;
    s.per_wave = 64u * 8u + s.batches * 16u + 64u + s.rowb;
    return s;
}

// what one lane wrote to LDS, every lane of the SAME wavefront may read afterwards
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ u64 below(unsigned lane) { return (1ull << lane) - 1ull; }   // the lanes in front of this one

// NOISE(qp, sine, cosine): one of the three policies of assoc_noise.h; qp: meas_var, Q, or the detections' Q_k
template <bool CREATE, class NOISE, class QP> __device__ __forceinline__ void associate_body(const AssocArgs& a, const QP& qp)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;   // (no workgroup barrier below: a wavefront is on its own)
    const unsigned L = (unsigned)a.nlandmarks, K = (unsigned)a.ndet;
    const AssocLds lds = assoc_lds(L);
    unsigned char* mine = smem + (unsigned)wave * lds.per_wave;
    u64* s_best = reinterpret_cast<u64*>(mine);
    u64* s_unseen = s_best + 64;
    unsigned char* s_fresh = reinterpret_cast<unsigned char*>(s_unseen + 2u * lds.batches);
    unsigned char* s_row = s_fresh + 64;
    unsigned* s_row32 = reinterpret_cast<unsigned*>(s_row);

    s_best[lane] = ~0ull;
    for (unsigned d = lane; d < lds.rowb / 4u; d += 64u) s_row32[d] = 0xffffffffu;

    const int src = a.anc ? a.anc[i] : i;
    float st, ct;
    det_sincosf(a.th[i], st, ct);
    const float px = a.x[i], py = a.y[i];
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t rin = row_rsrc(a.map, src, a.row_stride, row_bytes);
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    // a. lane k: detection k in the world frame (the observed point of ekf_particle / ekf_first_sighting)
    const float zxk = lane < K ? a.det_zx[lane] : 0.0f, zyk = lane < K ? a.det_zy[lane] : 0.0f;
    float wxk, wyk;
    ekf_first_sighting<float>(zxk, zyk, st, ct, px, py, wxk, wyk);

    const NOISE noise(qp, st, ct);
    const float inf = __uint_as_float(0x7f800000u);
    bool near = false;   // lane k: some seen landmark lies within new_gate of detection k
    for (unsigned b = 0; b < lds.batches; ++b) {
        v2f m[5];
        unsigned l[2];
        bool in[2], seen[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            l[t] = b * 128u + 64u * t + lane;
            in[t] = l[t] < L;
            const unsigned off = (in[t] ? l[t] : 0u) * 4u;   // clamped index + select instead of a predicated load
#pragma unroll
            for (int p = 0; p < 5; ++p) m[p][t] = row_load(rin, off, p * pl);
        }
        v2f mx = m[0];
        const v2f my = m[1], pxx = m[2], pxy = m[3], pyy = m[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            seen[t] = in[t] && !(pxx[t] < 0.0f);   // the update's own first-sighting test
            const u64 unseen = __ballot(in[t] && pxx[t] < 0.0f);
            if (lane == 0) s_unseen[2u * b + t] = unseen;
            // a landmark that takes no part: NaN in its mean makes every m NaN, and NaN passes none of the comparisons below
            mx[t] = seen[t] ? mx[t] : __uint_as_float(0x7fc00000u);
        }
        // b. S^-1, once per landmark — or, under a covariance per detection, per pair inside the loop
        EkfShared<v2f> h;
        if constexpr (!NOISE::kPerDetection) h = noise.inverse(pxx, pxy, pyy);
        // c. the cheapest detection of each landmark
        v2f best = bc2(inf);
        unsigned bk[2] = { 0u, 0u };
        for (unsigned k = 0; k < K; ++k) {
            const v2f wx = bc2(lane_value(wxk, (int)k)), wy = bc2(lane_value(wyk, (int)k));
            if constexpr (NOISE::kPerDetection) h = noise.inverse(pxx, pxy, pyy, k);
            const v2f dx = wx - mx, dy = wy - my;
            const v2f t0 = h.i00 * dx + h.i01 * dy, t1 = h.i01 * dx + h.i11 * dy;
            const v2f maha = dx * t0 + dy * t1;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const bool take = maha[t] < best[t];
                best[t] = take ? maha[t] : best[t];
                bk[t] = take ? k : bk[t];
            }
            if (CREATE) {   // lane k keeps detection k's flag
                const bool any = __builtin_amdgcn_ballot_w64(maha[0] <= a.new_gate || maha[1] <= a.new_gate) != 0;
                near = (lane == k && any) ? true : near;
            }
        }
        // d. candidates post to their detection's minimum
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (seen[t] && best[t] >= 0.0f && best[t] <= a.gate) {
                const unsigned bits = best[t] == 0.0f ? 0u : __float_as_uint(best[t]);   // -0 -> +0
                atomicMin(&s_best[bk[t]], ((u64)bits << 32) | l[t]);
            }
    }
    wave_lds_sync();

    const u64 won = s_best[lane];
    const bool matched = lane < K && won != ~0ull;
    if (matched) s_row[(unsigned)won] = (unsigned char)lane;
    const int nmatched = __popcll(__ballot(matched));
    int ncreated = 0;
    if (CREATE) {
        // e. the new detections in ascending k -> fresh[0 .. nfresh), then the unseen slots in ascending l take them in turn
        const bool fresh = lane < K && !matched && !near;
        const u64 fm = __ballot(fresh);
        const int nfresh = __popcll(fm);
        if (fresh) s_fresh[__popcll(fm & below(lane))] = (unsigned char)lane;
        wave_lds_sync();
        int taken = 0;   // unseen slots in the words walked so far
        for (unsigned w = 0; w < 2u * lds.batches && taken < nfresh; ++w) {
            const u64 um = s_unseen[w];
            const int rank = taken + __popcll(um & below(lane));
            if (((um >> lane) & 1ull) && rank < nfresh) s_row[64u * w + lane] = s_fresh[rank];
            taken += __popcll(um);
        }
        ncreated = taken < nfresh ? taken : nfresh;
    }
    if (lane == 0 && a.stats) {
        int32_t* st3 = a.stats + 3 * (size_t)i;
        st3[0] = nmatched;
        st3[1] = ncreated;
        st3[2] = (int)K - nmatched - ncreated;
    }
    wave_lds_sync();

    // the row: [0, rowb) from LDS (255 from L on), the rest of the stride 255
    const unsigned stride = (unsigned)a.assoc_stride;
    uint8_t* out = a.assoc + (size_t)i * stride;
    if ((stride & 3u) == 0 && (reinterpret_cast<uintptr_t>(a.assoc) & 3u) == 0) {   // (wave-uniform) every row starts on a dword
        unsigned* out32 = reinterpret_cast<unsigned*>(out);
        for (unsigned d = lane; d < stride / 4u; d += 64u) out32[d] = d < lds.rowb / 4u ? s_row32[d] : 0xffffffffu;
    } else {
        for (unsigned c = lane; c < stride; c += 64u) out[c] = c < lds.rowb ? s_row[c] : (uint8_t)255;
    }
}

template <bool CREATE> __global__ __launch_bounds__(kEkfWaves * 64) void associate_kernel(AssocArgs a)
{
    associate_body<CREATE, AssocNoiseIso>(a, a.meas_var);
}

// ... under S = P + R_w (a.meas_var is not read)
template <bool CREATE> __global__ __launch_bounds__(kEkfWaves * 64) void associate_aniso_kernel(AssocArgs a, EkfAnisoCov q)
{
    associate_body<CREATE, AssocNoiseAniso>(a, q);
}

// ... under S = P + R_w(k), Q_k per detection (a.meas_var is not read)
template <bool CREATE> __global__ __launch_bounds__(kEkfWaves * 64) void associate_detcov_kernel(AssocArgs a, DetCovArgs q)
{
    associate_body<CREATE, AssocNoiseDet>(a, q);
}

// the shapes the LDS carve and the row accesses of the associating kernels are sized by
bool assoc_args_ok(const AssocArgs& a)
{
    return !(a.nlandmarks < 0 || a.nlandmarks > SLAM_MAX_OBS || a.ndet < 0 || a.ndet > SLAM_MAX_DETECTIONS ||
             a.assoc_stride < a.nlandmarks || a.plane_stride < a.nlandmarks);
}

}  // namespace

hipError_t launch_associate(hipStream_t stream, const AssocArgs& a_in, const EkfAnisoCov* q, bool create, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!assoc_args_ok(a_in) || (q && !ekf_aniso_cov_ok(*q))) return hipErrorInvalidValue;
    AssocArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const size_t lds = (size_t)kEkfWaves * assoc_lds((unsigned)a.nlandmarks).per_wave;   // at most 4 x 9 792 bytes
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (q) {
        if (create) associate_aniso_kernel<true><<<blocks, kEkfWaves * 64, lds, stream>>>(a, *q);
        else associate_aniso_kernel<false><<<blocks, kEkfWaves * 64, lds, stream>>>(a, *q);
    } else {
        if (create) associate_kernel<true><<<blocks, kEkfWaves * 64, lds, stream>>>(a);
        else associate_kernel<false><<<blocks, kEkfWaves * 64, lds, stream>>>(a);
    }
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_associate_detcov(hipStream_t stream, const AssocArgs& a_in, const DetCovArgs& q, bool create, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!assoc_args_ok(a_in) || q.ndet != a_in.ndet || (q.ndet > 0 && (!q.qxx || !q.qxy || !q.qyy))) return hipErrorInvalidValue;
    AssocArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const size_t lds = (size_t)kEkfWaves * assoc_lds((unsigned)a.nlandmarks).per_wave;
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (create) associate_detcov_kernel<true><<<blocks, kEkfWaves * 64, lds, stream>>>(a, q);
    else associate_detcov_kernel<false><<<blocks, kEkfWaves * 64, lds, stream>>>(a, q);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
