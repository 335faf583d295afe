// assoc_kernels.hip — data association (no counterpart in the reference; specification: tests/_assoc_spec.py, DESIGN.md
// section 7): the detections of a frame are sensor-frame points without identity, and every particle decides for itself which of
// its landmarks each one belongs to and which ones start a new landmark (associate_kernel); the landmark update then reads its
// observations through the particle's table (ekf_update_kernel of ekf_kernels.hip with EkfObsTable as its source of z).
// Rows only: a table per particle means "which landmarks a frame observes" differs between particles, which the split, paged
// and grouped forms rely on being the same.
//
// associate_kernel: the matching of match_body.h (a wavefront per particle; steps a, c, d and the table row are its functions)
// on the particle's OWN ROW, read through a buffer resource in the access shape of ekf_row_body.h, under one of the noise
// policies of assoc_noise.h (step b: meas_var * I, a full 2x2 Q, or a Q_k per detection).  What is the association's own:
//   - seen and unseen: a slot with P_xx < 0 gets the NaN mean that keeps it out of the matching, and its bit in a 64-bit
//     "unseen" mask per 64 landmarks;
//   e. a detection that matched nothing and lies within new_gate of no seen landmark (a flag per detection, from a ballot
//      beside step c, kept by lane k) takes the next unseen slot: the ranks come from popcounts over the unseen masks.

#include "assoc_noise.h"
#include "match_body.h"

namespace slam {

namespace {

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
    match_reset(s_best, s_row, lds.rowb, lane);

    const int src = a.anc ? a.anc[i] : i;
    float st, ct;
    det_sincosf(a.th[i], st, ct);
    const float px = a.x[i], py = a.y[i];
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t rin = row_rsrc(a.map, src, a.row_stride, row_bytes);
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    float wxk, wyk;
    match_world_point(a.det_zx, a.det_zy, K, lane, st, ct, px, py, wxk, wyk);

    const NOISE noise(qp, st, ct);
    const float inf = __uint_as_float(0x7f800000u);
    bool near = false;   // lane k: some seen landmark lies within new_gate of detection k
    for (unsigned b = 0; b < lds.batches; ++b) {
        v2f m[5];
        const unsigned l0 = b * 128u + lane;
        bool in[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            in[t] = l0 + 64u * t < L;
            const unsigned off = (in[t] ? l0 + 64u * t : 0u) * 4u;   // clamped index + select instead of a predicated load
#pragma unroll
            for (int p = 0; p < 5; ++p) m[p][t] = row_load(rin, off, p * pl);
        }
        v2f mx = m[0];
        const v2f my = m[1], pxx = m[2], pxy = m[3], pyy = m[4];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool seen = in[t] && !(pxx[t] < 0.0f);   // the update's own first-sighting test
            const u64 unseen = __ballot(in[t] && pxx[t] < 0.0f);
            if (lane == 0) s_unseen[2u * b + t] = unseen;
            mx[t] = seen ? mx[t] : __uint_as_float(0x7fc00000u);   // (takes no part: match_body.h)
        }
        // b. S^-1, once per landmark — or, under a covariance per detection, per pair inside the loop
        EkfShared<v2f> h;
        if constexpr (!NOISE::kPerDetection) h = noise.inverse(pxx, pxy, pyy);
        v2f best = bc2(inf);
        unsigned bk[2] = { 0u, 0u };
        for (unsigned k = 0; k < K; ++k) {
            v2f wx, wy;
            match_point(wxk, wyk, k, wx, wy);
            if constexpr (NOISE::kPerDetection) h = noise.inverse(pxx, pxy, pyy, k);
            const v2f maha = match_pair(wx, wy, k, mx, my, h, best, bk);
            if (CREATE) {   // lane k keeps detection k's flag
                const bool any = __builtin_amdgcn_ballot_w64(maha[0] <= a.new_gate || maha[1] <= a.new_gate) != 0;
                near = (lane == k && any) ? true : near;
            }
        }
        match_post(s_best, best, bk, a.gate, l0);
    }
    wave_lds_sync();

    const MatchWinner won = match_winner(s_best, lane, K);
    const bool matched = won.matched;
    if (matched) s_row[won.l] = (unsigned char)lane;
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

    match_row_write(s_row, lds.rowb, a.assoc, i, (unsigned)a.assoc_stride, lane);
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

hipError_t launch_associate(hipStream_t stream, const AssocArgs& a_in, const EkfAnisoCov* q, const DetCovArgs* dq, bool create, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!assoc_args_ok(a_in) || (q && dq) || (q && !ekf_aniso_cov_ok(*q)) ||
        (dq && (dq->ndet != a_in.ndet || (dq->ndet > 0 && (!dq->qxx || !dq->qxy || !dq->qyy)))))
        return hipErrorInvalidValue;
    AssocArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const size_t lds = (size_t)kEkfWaves * assoc_lds((unsigned)a.nlandmarks).per_wave;   // at most 4 x 9 792 bytes
    const auto launch = [&](auto kernel, const auto&... noise) {
        if (ev) (void)hipEventRecord(ev->start, stream);
        kernel<<<blocks, kEkfWaves * 64, lds, stream>>>(a, noise...);
        if (ev) (void)hipEventRecord(ev->stop, stream);
    };
    if (dq) create ? launch(associate_detcov_kernel<true>, *dq) : launch(associate_detcov_kernel<false>, *dq);
    else if (q) create ? launch(associate_aniso_kernel<true>, *q) : launch(associate_aniso_kernel<false>, *q);
    else create ? launch(associate_kernel<true>) : launch(associate_kernel<false>);
    return hipGetLastError();
}

}  // namespace slam
