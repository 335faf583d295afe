// evidence_kernels.hip — landmark existence evidence (no counterpart in the reference; specification: tests/_evidence_spec.py,
// DESIGN.md section 7): every particle keeps one evidence byte c in [0, cmax] per landmark slot beside its row.  Behind the
// update of a frame (ekf_assoc_kernel) a landmark that took a detection gains `hit`; one that took none although it lies within
// view_range of the particle's pose loses `miss`; one that cannot pay the miss is PRUNED — its slot gets the bits of a slot that
// was never used (0, 0, -1, 0, 0), so the association hands it out again — and a clutter detection no longer keeps a slot for good.
//
// Two rules spare a landmark that is due a miss (seen, not hit, within view_range); either, both or neither may be on:
//   FOV (specification: tests/_fov_spec.py): its direction in the sensor frame lies OUTSIDE the arc [lo, hi] of the diamond angle
//   — the reference's lidar sees 269.5 degrees, and a landmark that drifts into the blind quarter behind the robot is not missing,
//   it is not looked at.  A hit counts whatever the direction.
//   SIGHT (specification: tests/_sight_spec.py; the table: sight_kernels.hip): it lies BEHIND what the frame's scan hit in its
//   direction — the nearest return of its bin and the two neighbours is closer than (r - margin)^2.  The arc test comes first.
//
// evidence_stage_kernel<WIDE, FOV, SIGHT>, one body for every form: ONE WAVEFRONT OWNS ONE PARTICLE, lanes own landmarks l and
// l + 64 of each batch of 128 (the access shape of ekf_row_body.h, the grid and row resources of associate_kernel).  Per landmark
// it reads three planes of the row (12 B), the table byte and the evidence byte, and writes one byte; only a prune, which is
// rare, writes the five floats of the slot.
// The predicate — due, in view, hidden — is evidence_visibility of evidence_common.h, which the localise stage's misses call too.
// FOV || SIGHT: the heading is read and, only in wavefronts in which some lane is due a miss, the offset is rotated into the
// sensor frame and its diamond angle taken (one division).  SIGHT: the table is staged once per workgroup in LDS (at most 4 KB:
// eight workgroups of a CU hold 32 KB of its 160; the workgroup's only barrier behind it), and the square root and the three
// table reads run only where some lane is due a miss AND in view.  The results depend on neither skip.  Neither switch on: no
// heading is read (sg.th may be nullptr), no LDS, no barrier.
// Byte traffic: 64 byte accesses of a wavefront move 64 B per instruction.  WIDE (every row of the three byte arrays starts on a
// dword: strides multiples of 4, bases aligned — decided by the launcher) moves the bytes of a batch as dwords instead: lanes
// 0..31 load the 32 dwords of the table, lanes 32..63 those of the evidence in the SAME instruction, every lane picks its bytes
// out of a neighbour's dword with a lane read, and the new bytes are packed back (an OR over the four lanes of a dword, one lane
// read to put the dwords in order) and leave as one 128-byte store.  The byte form stays for every other stride or base.
// The row is never read through a predicated load beyond nlandmarks: a clamped index plus a select, as elsewhere.
// evidence_init_kernel: c = seen ? value : 0 for whole rows (the same lanes, packing and stores).  evidence_gather_kernel:
// out[i] = in[anc[i]], whole rows of bytes (a frame without a landmark update: the evidence follows its particles).

#include "evidence_common.h"

namespace slam {

namespace {

template <bool WIDE, bool FOV, bool SIGHT>
__global__ __launch_bounds__(kEkfWaves * 64) void evidence_stage_kernel(EvidenceArgs a, SightArgs sg, FovArgs fv)
{
    constexpr bool DIR = FOV || SIGHT;   // the landmark's direction in the sensor frame is needed
    __shared__ float s_tab[SIGHT ? kSightMaxBins : 1];
    if (SIGHT) {
        for (int j = (int)threadIdx.x; j < sg.bins; j += kEkfWaves * 64) s_tab[j] = sg.table[j];
        __syncthreads();
    }
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;   // (SIGHT: behind the workgroup's only barrier; from here a wavefront is on its own)
    const unsigned L = (unsigned)a.nlandmarks, K = (unsigned)a.ndet;
    const unsigned hit = (unsigned)a.hit, miss = (unsigned)a.miss, cmax = (unsigned)a.cmax;
    const bool in_place = a.ev_in == a.ev_out;
    const int src = a.anc ? a.anc[i] : i;
    const float px = a.x[i], py = a.y[i];
    float sn = 0.0f, cs = 1.0f;
    if (DIR) det_sincosf(sg.th[i], sn, cs);
    const EvidenceView ev{ px, py, sn, cs, a.range2, fv.lo, fv.hi, fv.lo > fv.hi, s_tab, (float)(sg.bins >> 2), (unsigned)sg.bins - 1u, sg.margin };
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
    int npruned = 0, nseen = 0, nmissed = 0, nspared = 0, noutside = 0;
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
        bool seen[2], hit_now[2], open[2], due[2], view[2], hidden[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            seen[t] = in[t] && !(m[2][t] < 0.0f);   // the update's own first-sighting test: -0 counts as seen
            hit_now[t] = tk[t] < K;                  // a byte that names no detection of this frame is no hit
            open[t] = seen[t] && !hit_now[t];        // due a miss unless out of range, outside or hidden
        }
        evidence_visibility<2>(ev, FOV, SIGHT, m[0], m[1], open, due, view, hidden);
        unsigned cn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool outside = due[t] && !view[t];
            const bool missed = due[t] && view[t] && !hidden[t];
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
            if (SIGHT) nspared += __popcll(__ballot(hidden[t]));
            if (FOV) noutside += __popcll(__ballot(outside));
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
        if (DIR && sg.spared) sg.spared[i] = nspared;   // (FOV without SIGHT: nothing is hidden, 0)
        if (FOV && fv.outside) fv.outside[i] = noutside;
    }
}

template <bool WIDE>
__global__ __launch_bounds__(kEkfWaves * 64) void evidence_init_kernel(EvidenceInitArgs a)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.nrows) return;
    const unsigned L = (unsigned)a.nlandmarks;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t row = row_rsrc(a.map, i, a.row_stride, row_bytes);
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    guchar* cout = (guchar*)(uniform_gptr(a.ev + (size_t)i * (size_t)a.ev_stride));
    const unsigned batches = (L + 127u) / 128u;
    for (unsigned b = 0; b < batches; ++b) {
        unsigned cn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = b * 128u + 64u * t + lane;
            const bool in = l < L;
            const float pxx = row_load(row, (in ? l : 0u) * 4u, 2 * pl);
            cn[t] = in && !(pxx < 0.0f) ? (unsigned)a.value : 0u;
            if (!WIDE && in) cout[l] = (uint8_t)cn[t];
        }
        if (WIDE) batch_store((guint*)cout, b, lane, cn[0], cn[1], (unsigned)a.ev_stride / 4u);
    }
    zero_tail<WIDE>(cout, WIDE ? batches * 128u : L, (unsigned)a.ev_stride, lane);
}

template <bool WIDE>
__global__ __launch_bounds__(kEkfWaves * 64) void evidence_gather_kernel(const uint8_t* in, uint8_t* out, int stride, const int32_t* anc,
                                                                          int n, int xcd_chunk)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(xcd_chunk) * kEkfWaves + wave;
    if (i >= n) return;
    const guchar* src = (const guchar*)(uniform_gptr(in + (size_t)anc[i] * (size_t)stride));
    guchar* dst = (guchar*)(uniform_gptr(out + (size_t)i * (size_t)stride));
    if (WIDE) {
        const guint* s32 = (const guint*)src;
        guint* d32 = (guint*)dst;
        for (unsigned d = lane; d < (unsigned)stride / 4u; d += 64u) d32[d] = s32[d];
    } else {
        for (unsigned c = lane; c < (unsigned)stride; c += 64u) dst[c] = src[c];
    }
}

}  // namespace

bool fov_bounds_ok(float lo, float hi) { return lo >= 0.0f && lo <= 4.0f && hi >= 0.0f && hi <= 4.0f; }   // (NaN fails)

template <bool FOV, bool SIGHT>
static void (*evidence_stage(bool wide))(EvidenceArgs, SightArgs, FovArgs)
{
    return wide ? evidence_stage_kernel<true, FOV, SIGHT> : evidence_stage_kernel<false, FOV, SIGHT>;
}

hipError_t launch_landmark_evidence(hipStream_t stream, const EvidenceArgs& a_in, const SightArgs* sg, const FovArgs* fv, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    const bool fov = fv != nullptr;
    const bool sight = sg && (!fov || sg->table);   // under a field of view, no table: without line of sight
    // what the row, byte and LDS accesses are sized by, each part for the form that needs it
    if (!evidence_args_ok(a_in) || (fov && (!sg || !fov_bounds_ok(fv->lo, fv->hi))) || (sg && !sg->th) ||
        (sight && (!sg->table || !sight_bins_ok(sg->bins) || !(sg->margin > 0.0f))))
        return hipErrorInvalidValue;
    EvidenceArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const bool wide = dword_rows(a.assoc, a.assoc_stride) && dword_rows(a.ev_in, a.ev_stride) && dword_rows(a.ev_out, a.ev_stride);
    const auto kernel = fov ? (sight ? evidence_stage<true, true>(wide) : evidence_stage<true, false>(wide))
                            : (sight ? evidence_stage<false, true>(wide) : evidence_stage<false, false>(wide));
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a, sg ? *sg : SightArgs{}, fv ? *fv : FovArgs{});
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_evidence_init(hipStream_t stream, const EvidenceInitArgs& a_in, const EventPair* ev)
{
    if (a_in.nrows <= 0) return hipSuccess;
    if (a_in.nlandmarks < 0 || a_in.ev_stride < a_in.nlandmarks || a_in.plane_stride < a_in.nlandmarks || a_in.value < 0 || a_in.value > 255)
        return hipErrorInvalidValue;
    EvidenceInitArgs a = a_in;
    const int blocks = xcd_grid(a.nrows, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (dword_rows(a.ev, a.ev_stride)) evidence_init_kernel<true><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else evidence_init_kernel<false><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_evidence_gather(hipStream_t stream, const uint8_t* in, uint8_t* out, int stride, const int32_t* anc, int n)
{
    if (n <= 0 || stride <= 0) return hipSuccess;
    if (!in || !out || !anc || in == out) return hipErrorInvalidValue;
    int chunk = 0;
    const int blocks = xcd_grid(n, kEkfWaves, chunk);
    if (dword_rows(in, stride) && dword_rows(out, stride)) evidence_gather_kernel<true><<<blocks, kEkfWaves * 64, 0, stream>>>(in, out, stride, anc, n, chunk);
    else evidence_gather_kernel<false><<<blocks, kEkfWaves * 64, 0, stream>>>(in, out, stride, anc, n, chunk);
    return hipGetLastError();
}

}  // namespace slam
