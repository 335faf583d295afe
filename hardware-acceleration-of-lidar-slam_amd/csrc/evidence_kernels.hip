// evidence_kernels.hip — landmark existence evidence (no counterpart in the reference; specification: tests/_evidence_spec.py,
// DESIGN.md section 7): every particle keeps one evidence byte c in [0, cmax] per landmark slot beside its row.  Behind the
// update of a frame (ekf_assoc_kernel) a landmark that took a detection gains `hit`; one that took none although it lies within
// view_range of the particle's pose loses `miss`; one that cannot pay the miss is PRUNED — its slot gets the bits of a slot that
// was never used (0, 0, -1, 0, 0), so the association hands it out again — and a clutter detection no longer keeps a slot for good.
//
// evidence_kernel: ONE WAVEFRONT OWNS ONE PARTICLE, lanes own landmarks l and l + 64 of each batch of 128 (the access shape of
// ekf_row_body.h, the grid and row resources of associate_kernel).  Per landmark it reads three planes of the row (12 B), the
// table byte and the evidence byte, and writes one byte; only a prune, which is rare, writes the five floats of the slot.
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

template <bool WIDE>
__global__ __launch_bounds__(kEkfWaves * 64) void evidence_kernel(EvidenceArgs a)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;   // (no workgroup barrier below: a wavefront is on its own)
    const unsigned L = (unsigned)a.nlandmarks, K = (unsigned)a.ndet;
    const unsigned hit = (unsigned)a.hit, miss = (unsigned)a.miss, cmax = (unsigned)a.cmax;
    const bool in_place = a.ev_in == a.ev_out;
    const int src = a.anc ? a.anc[i] : i;
    const float px = a.x[i], py = a.y[i];
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
    int npruned = 0, nseen = 0, nmissed = 0;
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
        unsigned cn[2];
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool seen = in[t] && !(m[2][t] < 0.0f);   // the update's own first-sighting test: -0 counts as seen
            const bool hit_now = tk[t] < K;                  // a byte that names no detection of this frame is no hit
            const bool visible = evidence_r2(m[0][t], m[1][t], px, py) <= a.range2;   // (a NaN mean is not visible)
            const bool missed = seen && !hit_now && visible;
            const bool prune = missed && c[t] < miss;
            const unsigned up = c[t] + hit < cmax ? c[t] + hit : cmax;   // integers: 200 + 255 does not wrap
            unsigned v = seen && hit_now ? up : c[t];
            v = missed ? c[t] - miss : v;
            v = (prune || !seen) ? 0u : v;
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
            nseen += __popcll(__ballot(seen && !prune));
            nmissed += __popcll(__ballot(missed));
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

hipError_t launch_landmark_evidence(hipStream_t stream, const EvidenceArgs& a_in, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!evidence_args_ok(a_in))
        return hipErrorInvalidValue;   // what the row and byte accesses are sized by
    EvidenceArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    const bool wide = dword_rows(a.assoc, a.assoc_stride) && dword_rows(a.ev_in, a.ev_stride) && dword_rows(a.ev_out, a.ev_stride);
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (wide) evidence_kernel<true><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else evidence_kernel<false><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
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
