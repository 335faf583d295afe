// ekf_sparse_kernels.hip — the landmark update sparse in place behind the compact observation list.
// ---- sparse in-place form: frames that keep their population update only the OBSERVED landmarks, in place.
// Walking the rows in batches of 128 (ekf_batches, in place) runs the whole update arithmetic at full wavefront cost for
// the handful of lanes of a batch that hold an observation and touches every line a batch's observed landmarks lie in
// once per batch.  Here the observations are first compacted into a list sorted by landmark (once per observation
// table, build_obs_list_kernel); a wavefront then owns one particle and a LANE owns an observation (two per lane, as
// float2): gather the five values at that landmark, update, scatter them back — the same arithmetic in the same order.
// The log-likelihood keeps the summation order of the specification (landmark l adds to accumulator l mod 128 in order
// of l): the accumulators live in LDS, and observations that fall into the same accumulator carry a round number
// (how many earlier observations share it) and are added round by round.

#include "ekf_wave.h"
#include "storage_bodies.h"

namespace slam {

namespace {

// one workgroup: table (NaN = not observed) -> list in landmark order, rounds, counts (also to mapped host memory).
// L <= kObsListMaxLandmarks (the bitmap of observed landmarks lives in LDS).
__global__ __launch_bounds__(1024) void build_obs_list_kernel(const float* __restrict__ tzx, const float* __restrict__ tzy,
                                                              int L, ObsListOut ol, int32_t* __restrict__ h_count)
{
    __shared__ unsigned s_bits[kObsListMaxLandmarks / 32];
    __shared__ int s_wave[16];
    __shared__ int s_base;
    __shared__ int s_max_round;
    if (threadIdx.x == 0) { s_base = 0; s_max_round = 0; }
    __syncthreads();
    for (int l0 = 0; l0 < L; l0 += 1024) {   // ordered compaction, 1024 landmarks per step (storage_bodies.h)
        const int l = l0 + (int)threadIdx.x;
        const float vx = l < L ? tzx[l] : __builtin_nanf(""), vy = l < L ? tzy[l] : __builtin_nanf("");
        const bool ob = vx == vx && vy == vy;
        const unsigned long long m = __ballot(ob);
        obs_list_mark(m, l0, s_wave, s_bits);
        __syncthreads();
        obs_list_step(m, ob, l, vx, vy, s_wave, s_base, s_bits, ol, &s_max_round);
        __syncthreads();
        if (threadIdx.x == 0) {
            int tot = 0;
            for (int w = 0; w < 16; ++w) tot += s_wave[w];
            s_base += tot;
        }
        __syncthreads();
    }
    const int nobs = s_base;
    __syncthreads();
    if (threadIdx.x == 0) {
        ol.count[0] = nobs;
        ol.count[1] = s_max_round;
        if (h_count) {
            h_count[0] = nobs;
            h_count[1] = L;
        }
    }
}

__global__ __launch_bounds__(kEkfWaves * 64) void ekf_sparse_kernel(EkfArgs a, ObsListView ol)
{
    __shared__ float s_acc[kEkfWaves][128];
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;
    float st_, ct_;
    det_sincosf(a.th[i], st_, ct_);
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t row = row_rsrc(a.map_out, i, a.row_stride, row_bytes);   // in place: the particle's own row, read and written
    const v2f s = bc2(st_), c = bc2(ct_), px = bc2(a.x[i]), py = bc2(a.y[i]), q = bc2(a.meas_var);
    const int nobs = __builtin_amdgcn_readfirstlane(ol.count[0]);
    const int max_round = __builtin_amdgcn_readfirstlane(ol.count[1]);
    s_acc[wave][lane] = 0.0f;
    s_acc[wave][lane + 64] = 0.0f;
    for (int k0 = 0; k0 < nobs; k0 += 128) {
        bool ob[2];
        unsigned off[2];
        int slot[2], rnd[2];
        v2f zx, zy, m[5];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int k = k0 + 64 * t + (int)lane;
            ob[t] = k < nobs;
            const int kk = ob[t] ? k : 0;
            const int l = ol.id[kk];
            off[t] = (unsigned)l * 4u;
            slot[t] = l & 127;
            rnd[t] = ol.round[kk];
            zx[t] = ol.zx[kk];
            zy[t] = ol.zy[kk];
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int p = 0; p < 5; ++p) m[p][t] = ob[t] ? row_load(row, off[t], p * pl) : 1.0f;   // 1: harmless operands for idle lanes
        const v2f mx = m[0], my = m[1], pxx = m[2], pxy = m[3], pyy = m[4];
        const EkfResult<v2f> u = ekf_update_one<v2f>(mx, my, pxx, pxy, pyy, zx, zy, s, c, px, py, q);
        const v2f o0 = u.o0, o1 = u.o1, o2 = u.o2, o3 = u.o3, o4 = u.o4, f0 = u.f0, f1 = u.f1, ll = u.ll;
        float term[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool first = pxx[t] < 0.0f;
            term[t] = first ? 0.0f : ll[t];
            if (ob[t]) {
                row_store(row, off[t], 0 * pl, first ? f0[t] : o0[t]);
                row_store(row, off[t], 1 * pl, first ? f1[t] : o1[t]);
                row_store(row, off[t], 2 * pl, first ? q[t] : o2[t]);
                row_store(row, off[t], 3 * pl, first ? 0.0f : o3[t]);
                row_store(row, off[t], 4 * pl, first ? q[t] : o4[t]);
            }
        }
        // log-likelihood: accumulator = landmark mod 128, in order of the landmark: round by round (observations of one
        // accumulator have distinct rounds; a wavefront's LDS operations execute in order)
        for (int r = 0; r <= max_round; ++r)
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (ob[t] && rnd[t] == r) s_acc[wave][slot[t]] = s_acc[wave][slot[t]] + term[t];
    }
    const float total = wave_xor_tree_sum(s_acc[wave][lane] + s_acc[wave][lane + 64]);
    if (lane == 0) store_loglik(a, i, total);
}
}  // namespace

hipError_t launch_build_obs_list(hipStream_t stream, const float* tzx, const float* tzy, int L, const ObsListOut& ol, int32_t* h_count)
{
    build_obs_list_kernel<<<1, 1024, 0, stream>>>(tzx, tzy, L, ol, h_count);
    return hipGetLastError();
}

hipError_t launch_ekf_sparse(hipStream_t stream, const EkfArgs& a_in, const ObsListView& ol, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    EkfArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    ekf_sparse_kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a, ol);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
