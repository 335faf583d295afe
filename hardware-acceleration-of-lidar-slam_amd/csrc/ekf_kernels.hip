// ekf_kernels.hip — the motion sample and the landmark update of the particle filter: the 2x2 EKF
// per (particle, landmark) with a row per wavefront (in its five forms: noise meas_var * I or a 2x2 Q, observations from the
// frame's table or through a per-particle association table — and, through the table, a Q per detection), grouped and on
// the split layout (the bodies: ekf_row_body.h, ekf_aniso_lane.h, ekf_group_body.h, ekf_split_body.h; what they share and
// the data layout: ekf_wave.h), plus the copy ceiling and the reciprocal self-test.  Fused with the scorer into the front of a
// frame: front_kernels.hip; sparse in place behind the compact observation list: ekf_sparse_kernels.hip.  The only reference
// anchor is the zero-noise motion step = the constant-velocity predict of Subsystem_1/main.c:875-898.

#include "ekf_aniso_lane.h"
#include "ekf_group_body.h"
#include "ekf_split_body.h"

namespace slam {

namespace {

// ------------------------------------------------------------------ A9: motion sample
__global__ __launch_bounds__(kBlock) void motion_sample_kernel(const float* __restrict__ sx,
                                                               const float* __restrict__ sy,
                                                               const float* __restrict__ sth,
                                                               const int32_t* __restrict__ anc, float* __restrict__ x,
                                                               float* __restrict__ y, float* __restrict__ th, int n,
                                                               MotionParams mp)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = anc ? anc[i] : i;
    float ox, oy, ot;
    motion_sample_one(mp, (uint64_t)i, sx[j], sy[j], sth[j], ox, oy, ot);
    x[i] = ox;
    y[i] = oy;
    th[i] = ot;
}

// ------------------------------------------------------------------ A10: 2x2 EKF per (particle, landmark)
// One wavefront per particle walks its row.  NB: batches of 128 landmarks per pass of the fast path.  COPY: out of place.
// NOISE, OBS: the two policies of ekf_row_body.h, each with the argument it needs beyond EkfArgs.
template <int NB, bool COPY, class NOISE, class OBS>
__global__ __launch_bounds__(kEkfWaves * 64) void ekf_update_kernel(EkfArgs a, typename NOISE::Args na, typename OBS::Args oa)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;
    const int src = a.anc ? a.anc[i] : i;
    float st_, ct_;
    det_sincosf(a.th[i], st_, ct_);
    EkfRowLane<NOISE, OBS> w;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    w.rin = row_rsrc(a.map_in, src, a.row_stride, row_bytes);
    w.p.rout = row_rsrc(a.map_out, i, a.row_stride, row_bytes);
    w.pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    w.L = (unsigned)a.nlandmarks;
    w.p.s = bc2(st_); w.p.c = bc2(ct_); w.p.px = bc2(a.x[i]); w.p.py = bc2(a.y[i]);
    w.noise.init(a, na, st_, ct_);
    w.obs.init(a, oa, i, lane);

    const float total = ekf_row_walk<NB, COPY>(w, (unsigned)a.plane_stride, lane);
    if (lane == 0) store_loglik(a, i, total);
}

template <int NB, int G>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(kEkfGroupWpe, kEkfGroupWpe)))
void ekf_update_group_kernel(EkfArgs a)
{
    __shared__ float s_acc[kEkfWaves][G][128];
    ekf_group_body<NB, G, false>(a, xcd_block(a.xcd_chunk), s_acc, MotionIO{}, MotionParams{});
}

template <int NB, int G>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(kEkfSplitWpe, kEkfSplitWpe)))
void ekf_split_kernel(EkfArgs a)
{
    __shared__ float s_acc[kEkfWaves][G][128];
    ekf_split_body<NB, G, kPosesRead>(a, xcd_block(a.xcd_chunk), s_acc, MotionIO{}, MotionParams{});
}

// the mean rows of the split update alone (ekf_split_body, TALLY = false): survivor rows, launch_ekf_materialise
template <int NB, int G>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(kEkfSplitWpe, kEkfSplitWpe)))
void ekf_materialise_kernel(EkfArgs a)
{
    ekf_split_body<NB, G, kPosesRead, true, false>(a, xcd_block(a.xcd_chunk), nullptr, MotionIO{}, MotionParams{});
}

// ---- measurement support (slam_profile_copy_ceiling): the access shape of ekf_update_kernel without its arithmetic
__global__ __launch_bounds__(kEkfWaves * 64) void copy_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int n,
                                                                   int plane_stride, int xcd_chunk)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = threadIdx.x >> 6;
    const int i = xcd_block(xcd_chunk) * kEkfWaves + wave;
    if (i >= n) return;
    const float* rin = in + (size_t)i * 5 * plane_stride;
    float* rout = out + (size_t)i * 5 * plane_stride;
    for (int lb = 0; lb < plane_stride; lb += 256) {   // two batches of 128 landmarks: every load before the first store
        const int nb = plane_stride - lb >= 256 ? 2 : 1;
        float m[2][2][5];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int p = 0; p < 5; ++p)
                    if (g < nb) m[g][t][p] = rin[p * plane_stride + lb + g * 128 + t * 64 + lane];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int p = 0; p < 5; ++p)
                    if (g < nb) __builtin_nontemporal_store(m[g][t][p], &rout[p * plane_stride + lb + g * 128 + t * 64 + lane]);
    }
}

// every float whose exponent lies in the fast reciprocal's range (both signs): ekf_rcp_core against the compiler's IEEE
// division, the scalar form and the packed one; out[0] += mismatches, out[1] += values checked
__global__ __launch_bounds__(256) void selftest_reciprocal_kernel(unsigned long long* __restrict__ out)
{
    unsigned long long bad = 0, seen = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < (1ull << 32); b += (uint64_t)gridDim.x * 256) {
        const float d = __uint_as_float((uint32_t)b);
        if (!ekf_rcp_in_range(d)) continue;
        const float exact = 1.0f / d;
        const float fast = ekf_rcp_core(d);
        const v2f two = ekf_rcp((v2f){d, -d});   // (every lane here is in range: the packed fast path)
        bad += (__float_as_uint(exact) != __float_as_uint(fast)) || (__float_as_uint(two[0]) != __float_as_uint(exact)) ||
               (__float_as_uint(two[1]) != (__float_as_uint(exact) ^ 0x80000000u));
        ++seen;
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicAdd(&out[1], seen);
}
}  // namespace

hipError_t launch_motion_sample(hipStream_t stream, const float* sx, const float* sy, const float* sth,
                                const int32_t* anc, float* x, float* y, float* th, int n, int64_t first_id,
                                const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame)
{
    if (n <= 0) return hipSuccess;
    const MotionParams mp = make_motion_params(first_id, dp, sigma, seed, frame);
    motion_sample_kernel<<<blocks_for(n), kBlock, 0, stream>>>(sx, sy, sth, anc, x, y, th, n, mp);
    return hipGetLastError();
}

// one form of the row update: batches of 128 landmarks in flight per wavefront and the launch
template <class NOISE, class OBS>
static hipError_t launch_rows(hipStream_t stream, EkfArgs a, const typename NOISE::Args& na, const typename OBS::Args& oa, const EventPair* ev)
{
    const bool copy = a.map_in != a.map_out;   // in place: rows without an observation stay as they are
    const bool big = a.nlandmarks > 128;
    // out of place: 2 measured best at 64k x 500 (1: 178 us, 2: 166 us, 4: 180 us).  In place: 4 batches (512 landmarks) per round
    // trip; measured at 64k x 500 with 32 landmarks observed: 1 batch at a time 91 us, because every batch is its own dependent
    // chain obs table -> row -> store
    void (*kernel)(EkfArgs, typename NOISE::Args, typename OBS::Args);
    if (!copy) kernel = big ? ekf_update_kernel<4, false, NOISE, OBS> : ekf_update_kernel<1, false, NOISE, OBS>;
    else kernel = big ? ekf_update_kernel<2, true, NOISE, OBS> : ekf_update_kernel<1, true, NOISE, OBS>;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a, na, oa);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_ekf_rows(hipStream_t stream, const EkfArgs& a, const EkfAnisoCov* q, const EkfAssocTable* tab, const EventPair* ev)
{
    if (a.n <= 0) return hipSuccess;
    if (a.cov) return hipErrorInvalidValue;   // rows only
    if (tab && (tab->assoc_stride < a.nlandmarks || tab->ndet < 0 || tab->ndet > SLAM_MAX_DETECTIONS)) return hipErrorInvalidValue;
    if (q && !ekf_aniso_cov_ok(*q)) return hipErrorInvalidValue;
    if (q && tab) return launch_rows<EkfNoiseAniso, EkfObsTable>(stream, a, *q, *tab, ev);
    if (q) return launch_rows<EkfNoiseAniso, EkfObsFrame>(stream, a, *q, {}, ev);
    if (tab) return launch_rows<EkfNoiseIso, EkfObsTable>(stream, a, {}, *tab, ev);
    return launch_rows<EkfNoiseIso, EkfObsFrame>(stream, a, {}, {}, ev);
}

hipError_t launch_ekf_rows_detcov(hipStream_t stream, const EkfArgs& a, const DetCovArgs& q, const EkfAssocTable& tab, const EventPair* ev)
{
    if (a.n <= 0) return hipSuccess;
    if (a.cov || tab.assoc_stride < a.nlandmarks || tab.ndet < 0 || tab.ndet > SLAM_MAX_DETECTIONS || q.ndet != tab.ndet ||
        (q.ndet > 0 && (!q.qxx || !q.qxy || !q.qyy)))
        return hipErrorInvalidValue;
    return launch_rows<EkfNoiseDet, EkfObsTable>(stream, a, q, tab, ev);
}

hipError_t launch_ekf_update(hipStream_t stream, const EkfArgs& a_in, const EventPair* ev, int group_size)
{
    if (a_in.n <= 0) return hipSuccess;
    EkfArgs a = a_in;
    void (*kernel)(EkfArgs);   // the form, and how many particles a workgroup of it owns
    int per_block;
    const bool copy = a.map_in != a.map_out;   // in place: rows without an observation stay as they are
    if (a.cov) {   // split layout: always the grouped form (2 particles per wavefront unless the caller asks for 4 or 8)
        const int G = group_size == 4 || group_size == 8 ? group_size : 2;
        per_block = kEkfWaves * G;
        if (G == 8) kernel = ekf_split_kernel<kEkfSplitNb, 8>;
        else if (G == 4) kernel = ekf_split_kernel<kEkfSplitNb, 4>;
        else kernel = ekf_split_kernel<kEkfSplitNb, 2>;
    } else if (copy && a.nlandmarks > 128 && group_size > 0) {
        // out of place, more than one batch per row: optionally the grouped form (group_size neighbouring particles per
        // wavefront, shared source rows stay in registers); the caller knows roughly how many distinct ancestors the last
        // resample left (slam_ekf_form_set forces one form).
        // group size: measured on MI355X (64k x 500 | 1M x 1000 | 64k x 500 with 50 % distinct ancestors | 512k x 5000; one
        // wavefront per particle: 156 us | 4.28 ms | 177 us | 10.09 ms): 2 particles 148 | 4.09 | 169 | 9.79; 3: 135;
        // 4: 139 | 3.86 | 180 | 9.82; 6: 141; 8: 150 | 3.84 | 199 | 9.92.  Hence 4 when neighbours share ancestors, 2 when
        // they rarely do.  Batches in flight per pass (the first template argument),
        // group of 4, 64k x 500 | 1M x 1000 | 512k x 5000: 1: 150 us | 3.97 ms; 2: 140-145 | 3.90-3.92 | 9.79; 3: 144 | 4.02;
        // 4: 137-139 | 3.86 | 9.86 — within the run-to-run spread: 2 kept (82 VGPRs, 5 waves per SIMD; 4 needs 114).
        // The engine asks for 2 or 4 on rows (slam_engine::ekf_group_size); any other size gets the 4-particle kernel and its grid.
        const int G = group_size == 2 ? 2 : 4;
        per_block = kEkfWaves * G;
        if (G == 2) kernel = ekf_update_group_kernel<kEkfGroupNb, 2>;
        else kernel = ekf_update_group_kernel<kEkfGroupNb, 4>;
    } else {
        return launch_ekf_rows(stream, a, nullptr, nullptr, ev);   // one wavefront per particle
    }
    const int blocks = xcd_grid(a.n, per_block, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_ekf_materialise(hipStream_t stream, const EkfArgs& a_in, const EventPair* ev, int group_size)
{
    if (a_in.n <= 0) return hipSuccess;
    EkfArgs a = a_in;
    const int G = group_size == 4 || group_size == 8 ? group_size : 2;
    void (*kernel)(EkfArgs) = G == 8 ? ekf_materialise_kernel<kEkfSplitNb, 8>
                              : G == 4 ? ekf_materialise_kernel<kEkfSplitNb, 4> : ekf_materialise_kernel<kEkfSplitNb, 2>;
    const int blocks = xcd_grid(a.n, kEkfWaves * G, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_selftest_reciprocal(hipStream_t stream, unsigned long long* out)
{
    selftest_reciprocal_kernel<<<256 * 16, 256, 0, stream>>>(out);
    return hipGetLastError();
}

hipError_t launch_copy_rows(hipStream_t stream, const float* in, float* out, int n, int plane_stride)
{
    const int blocks = (n + kEkfWaves - 1) / kEkfWaves, chunk = (blocks + 7) / 8;
    copy_rows_kernel<<<chunk * 8, kEkfWaves * 64, 0, stream>>>(in, out, n, plane_stride, chunk);
    return hipGetLastError();
}

}  // namespace slam
