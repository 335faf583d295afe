// sight_kernels.hip — line of sight for the existence evidence (no counterpart in the reference; specification:
// tests/_sight_spec.py): a landmark that lies BEHIND what the frame's scan hit in its direction is hidden and
// takes no miss, so a pole that passes behind another pole or a wall keeps its slot, its mean and its covariance.
//
// Directions are `bins` (a power of two, 32 .. 1024) equal steps of the DIAMOND ANGLE p in [0, 4) of a sensor-frame point: with
// q = |y| / (|x| + |y|), p = q, 2 - q, 2 + q, 4 - q by quadrant — monotone in the true angle, one IEEE division, no arctangent.
// sight_table_kernel: ONE WORKGROUP, one launch over the engine's current scan (a latency kernel like the detector): an LDS table
// of `bins` words starts as +inf; every point takes the unsigned minimum of its bin with the bits of r2 = x*x + y*y (non-negative
// floats order as their bits, and a minimum does not depend on the order of arrival); one coalesced store of kSightMaxBins floats
// (+inf from `bins` on) to the engine's buffer.
// evidence_sight_kernel: evidence_kernel (evidence_kernels.hip: the same wavefront per particle, lanes, WIDE and byte paths,
// clamped loads and prune stores) with the table staged once per workgroup in LDS (at most 4 KB: eight workgroups of a CU hold
// 32 KB of its 160) and, for the landmarks that are due a miss, the hidden test: rotate the offset into the sensor frame, its bin,
// the nearest return of that bin and its two neighbours, against (r - margin)^2.  No lane of a wavefront due a miss: the wavefront
// skips the test (the results do not depend on it).

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

template <bool WIDE>
__global__ __launch_bounds__(kEkfWaves * 64) void evidence_sight_kernel(EvidenceArgs a, SightArgs sg)
{
    __shared__ float s_tab[kSightMaxBins];
    for (int j = (int)threadIdx.x; j < sg.bins; j += kEkfWaves * 64) s_tab[j] = sg.table[j];
    __syncthreads();
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;   // (behind the workgroup's only barrier: from here a wavefront is on its own)
    const unsigned L = (unsigned)a.nlandmarks, K = (unsigned)a.ndet;
    const unsigned hit = (unsigned)a.hit, miss = (unsigned)a.miss, cmax = (unsigned)a.cmax;
    const bool in_place = a.ev_in == a.ev_out;
    const int src = a.anc ? a.anc[i] : i;
    const float px = a.x[i], py = a.y[i];
    float sn, cs;
    det_sincosf(sg.th[i], sn, cs);
    const float quarter = (float)(sg.bins >> 2);
    const unsigned mask = (unsigned)sg.bins - 1u;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t row = row_rsrc(a.map, i, a.row_stride, row_bytes);   // read, and written where a landmark is pruned
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const guchar* tab = (const guchar*)(uniform_gptr(a.assoc + (size_t)i * (size_t)a.assoc_stride));
    const guchar* cin = (const guchar*)(uniform_gptr(a.ev_in + (size_t)src * (size_t)a.ev_stride));
    guchar* cout = (guchar*)(uniform_gptr(a.ev_out + (size_t)i * (size_t)a.ev_stride));
    const unsigned tab_dw = (unsigned)a.assoc_stride / 4u, ev_dw = (unsigned)a.ev_stride / 4u;   // WIDE: whole dwords per row
    // WIDE: the dwords that are stored — out of place every one of the row, in place those that hold a landmark
    const unsigned store_dw = in_place ? (L + 3u) / 4u : ev_dw;
    const unsigned batches = (L + 127u) / 128u;
    int npruned = 0, nseen = 0, nmissed = 0, nspared = 0;
    for (unsigned b = 0; b < batches; ++b) {
        unsigned tk[2], c[2];
        if (WIDE) {
            const bool second = lane >= 32u;
            const unsigned d = b * 32u + (lane & 31u);
            const guint* p = (const guint*)(second ? cin : tab);
            const unsigned w = p[d < (second ? ev_dw : tab_dw) ? d : 0u];   // clamped index: lanes beyond L discard what they get
            batch_bytes(w, lane, false, tk[0], tk[1]);
            batch_bytes(w, lane, true, c[0], c[1]);
        }
        unsigned l[2];
        bool in[2];
        float m[3][2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            l[t] = b * 128u + 64u * t + lane;
            in[t] = l[t] < L;
            const unsigned at = in[t] ? l[t] : 0u;   // clamped index + select instead of a predicated load
            if (!WIDE) {
                tk[t] = tab[at];
                c[t] = cin[at];
            }
#pragma unroll
            for (int p = 0; p < 3; ++p) m[p][t] = row_load(row, at * 4u, p * pl);
        }
        bool seen[2], hit_now[2], due[2], hidden[2];
        float r2[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            seen[t] = in[t] && !(m[2][t] < 0.0f);   // the update's own first-sighting test: -0 counts as seen
            hit_now[t] = tk[t] < K;                  // a byte that names no detection of this frame is no hit
            r2[t] = evidence_r2(m[0][t], m[1][t], px, py);
            due[t] = seen[t] && !hit_now[t] && r2[t] <= a.range2;   // due a miss unless hidden (a NaN mean is not visible)
            hidden[t] = false;
        }
        if (__ballot(due[0] || due[1])) {   // wave-uniform: the rotation, the division and the square root only where some lane needs them
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const float dx = m[0][t] - px, dy = m[1][t] - py;   // the visibility test's own dx, dy
                const float xa = cs * dx, xb = sn * dy;
                const float zx = xa - xb;                            // z = R(theta) (w - t)
                const float ya = sn * dx, yb = cs * dy;
                const float zy = ya + yb;
                unsigned j;
                const bool has = sight_bin(zx, zy, quarter, mask, j);
                const float near = fminf(fminf(s_tab[(j - 1u) & mask], s_tab[j]), s_tab[(j + 1u) & mask]);   // (no NaN in the table)
                const float r = sqrtf(r2[t]);   // correctly rounded (NOT __fsqrt_rn: det_math.h)
                const float g = r - sg.margin;
                const float g2 = g * g;
                hidden[t] = due[t] && has && g > 0.0f && near < g2;   // a NaN anywhere: not hidden
            }
        }
        unsigned cn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool missed = due[t] && !hidden[t];
            const bool prune = missed && c[t] < miss;
            const unsigned up = c[t] + hit < cmax ? c[t] + hit : cmax;   // integers: 200 + 255 does not wrap
            unsigned v = seen[t] && hit_now[t] ? up : c[t];
            v = missed ? c[t] - miss : v;
            v = (prune || !seen[t]) ? 0u : v;
            // beyond L: out of place the padding is written 0, in place it is left alone (WIDE: its own bytes go back)
            cn[t] = in[t] ? v : (in_place ? c[t] : 0u);
            if (prune) {   // rare: the five planes of a slot that was never used
                row_store(row, l[t] * 4u, 0 * pl, 0.0f);
                row_store(row, l[t] * 4u, 1 * pl, 0.0f);
                row_store(row, l[t] * 4u, 2 * pl, -1.0f);
                row_store(row, l[t] * 4u, 3 * pl, 0.0f);
                row_store(row, l[t] * 4u, 4 * pl, 0.0f);
            }
            if (!WIDE && in[t]) cout[l[t]] = (uint8_t)cn[t];
            npruned += __popcll(__ballot(prune));
            nseen += __popcll(__ballot(seen[t] && !prune));
            nmissed += __popcll(__ballot(missed));
            nspared += __popcll(__ballot(hidden[t]));
        }
        if (WIDE) batch_store((guint*)cout, b, lane, cn[0], cn[1], store_dw);
    }
    if (!in_place) zero_tail<WIDE>(cout, WIDE ? batches * 128u : L, (unsigned)a.ev_stride, lane);
    if (lane == 0) {
        if (a.stats) {
            int32_t* st2 = a.stats + 2 * (size_t)i;
            st2[0] = npruned;
            st2[1] = nseen;
        }
        if (a.missed) a.missed[i] = nmissed;
        if (sg.spared) sg.spared[i] = nspared;
    }
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

hipError_t launch_landmark_evidence_sight(hipStream_t stream, const EvidenceArgs& a_in, const SightArgs& sg, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!evidence_args_ok(a_in) || !sight_bins_ok(sg.bins) || !sg.table || !sg.th || !(sg.margin > 0.0f))
        return hipErrorInvalidValue;   // what the row, byte and LDS accesses are sized by
    EvidenceArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const bool wide = dword_rows(a.assoc, a.assoc_stride) && dword_rows(a.ev_in, a.ev_stride) && dword_rows(a.ev_out, a.ev_stride);
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (wide) evidence_sight_kernel<true><<<blocks, kEkfWaves * 64, 0, stream>>>(a, sg);
    else evidence_sight_kernel<false><<<blocks, kEkfWaves * 64, 0, stream>>>(a, sg);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
