// merge_kernels.hip — merging duplicate landmarks (no counterpart in the reference; specification: tests/_merge_spec.py,
// DESIGN.md section 7): two slots of one particle that hold the same pole become one.  Within a particle a detection updates
// exactly one landmark, so the two slots were fed disjoint sets of detections: given the particle's path they are independent
// estimates of one point, and their product — the general-covariance update of one with the other as "observed point" and
// "noise" (ekf_aniso_math.h) — is the posterior.  Behind the frame's associating update (and its evidence stage), in place.
//
// merge_kernel: ONE WAVEFRONT OWNS ONE PARTICLE, lanes own landmarks l and l + 64 of each batch of 128 (the access shape, grid
// and row resources of associate_kernel and evidence_stage_kernel).
//   1. roles: seen = !(P_xx < 0); an ANCHOR is seen and named by the frame's table (a_l < K: matched or created this frame), a
//      FREE landmark is seen and not named.  The anchors — at most K <= 64 under a table that names a detection once; of any
//      other table the first 64 — are compacted in ascending l by ballot and lane prefix into LDS: five values and the slot.
//      Lane j then keeps anchor j in registers.
//   2. the free landmark chooses: lanes walk the landmarks against the anchors in a wave-uniform loop as associate_kernel walks
//      them against the detections — S = P_l + P_w, S^-1 per pair with the update's own reciprocal, the Mahalanobis term of
//      d = mu_l - mu_w; strict <, j ascending: the lowest anchor on ties, NaN never wins.  Candidates (0 <= m <= gate) post
//      (bits(m) << 32 | l) to an LDS 64-bit minimum per anchor (step d of the association: -0 is made +0, l breaks ties).
//   3. the anchor chooses and absorbs: lane j reads the winner's five values from the row, fuses, and — unless the guard
//      refuses (a value that is not finite, P_xx <= 0, P_yy <= 0 or a float32 determinant <= 0 would turn the anchor into
//      garbage or into an unused slot) — writes the anchor, clears the absorbed slot to the bits of a slot that was never used,
//      and moves its evidence byte into the anchor's.
// NO READ-AFTER-WRITE HAZARD inside a particle: anchors are only ever rewritten, free slots are only ever cleared, a free slot
// chooses exactly one anchor and an anchor absorbs at most one slot, so the slots written in step 3 are pairwise distinct; every
// read of step 2 was consumed before the LDS hand-over in front of step 3, and in step 3 the lane that clears an absorbed slot
// is the one lane that read it, and it read it first.
// Byte traffic: the table is read as dwords (WIDE: every row starts on a dword — decided by the launcher) or as bytes; the
// evidence bytes of at most 64 pairs per particle move as bytes.  The row is never read through a predicated load beyond
// nlandmarks: a clamped index plus a select, as elsewhere.

#include "ekf_aniso_math.h"
#include "evidence_common.h"
#include "match_body.h"

namespace slam {

namespace {

typedef unsigned long long u64;

// the table bytes of landmarks l and l + 64 (l = 128 b + lane) of one particle
template <bool WIDE>
__device__ __forceinline__ void merge_table_bytes(const guchar* tab, unsigned tab_dw, unsigned b, unsigned lane, unsigned L, unsigned (&tk)[2])
{
    if (WIDE) {
        const unsigned d = b * 32u + (lane & 31u);
        const unsigned w = ((const guint*)tab)[d < tab_dw ? d : 0u];   // clamped index: lanes beyond L discard what they get
        batch_bytes(w, lane, false, tk[0], tk[1]);
    } else {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = b * 128u + 64u * t + lane;
            tk[t] = tab[l < L ? l : 0u];
        }
    }
}

// the absorbed landmark (lx, ly, lxx, lxy, lyy) into the anchor (mx, my, pxx, pxy, pyy): the operations of ekf_aniso_update_one
// with the observed point w = mu_l, R_w = P_l and detq = det P_l, without the likelihood term (tests/_merge_spec.py: fuse)
__device__ __forceinline__ void merge_fuse(float lx, float ly, float lxx, float lxy, float lyy, float mx, float my, float pxx, float pxy,
                                           float pyy, float (&o)[5])
{
    const float dx = lx - mx, dy = ly - my;
    const float a = pxx + lxx, b = pxy + lxy, cc = pyy + lyy;
    const float det = a * cc - b * b;
    const float idet = ekf_rcp(det);
    const float i00 = cc * idet, i01 = -b * idet, i11 = a * idet;            // S^-1
    const float t0 = i00 * dx + i01 * dy, t1 = i01 * dx + i11 * dy;          // S^-1 d
    o[0] = lx - (lxx * t0 + lxy * t1);
    o[1] = ly - (lxy * t0 + lyy * t1);
    const float detp = pxx * pyy - pxy * pxy;
    const float detl = lxx * lyy - lxy * lxy;
    o[2] = idet * (detp * lxx + detl * pxx);                                  // P_l S^-1 P_w
    o[3] = idet * (detp * lxy + detl * pxy);
    o[4] = idet * (detp * lyy + detl * pyy);
}

__device__ __forceinline__ bool merge_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

template <bool WIDE>
__global__ __launch_bounds__(kEkfWaves * 64) void merge_kernel(MergeArgs a)
{
    __shared__ u64 s_best_all[kEkfWaves][64];
    __shared__ float s_anchor_all[kEkfWaves][5][64];
    __shared__ unsigned s_slot_all[kEkfWaves][64];
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;   // (no workgroup barrier below: a wavefront is on its own)
    u64* s_best = s_best_all[wave];
    float(*s_anchor)[64] = s_anchor_all[wave];
    unsigned* s_slot = s_slot_all[wave];
    const unsigned L = (unsigned)a.nlandmarks, K = (unsigned)a.ndet;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t row = row_rsrc(a.map, i, a.row_stride, row_bytes);   // read, and written where a pair is merged
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const guchar* tab = (const guchar*)(uniform_gptr(a.assoc + (size_t)i * (size_t)a.assoc_stride));
    const unsigned tab_dw = (unsigned)a.assoc_stride / 4u;   // WIDE: whole dwords per row
    const unsigned batches = (L + 127u) / 128u;
    const u64 below = (1ull << lane) - 1ull;   // the lanes in front of this one

    s_best[lane] = ~0ull;
    // 1. roles; the anchors in ascending l -> LDS
    unsigned count = 0;
    int nseen = 0;
    for (unsigned b = 0; b < batches; ++b) {
        unsigned tk[2];
        merge_table_bytes<WIDE>(tab, tab_dw, b, lane, L, tk);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = b * 128u + 64u * t + lane;
            const bool in = l < L;
            const unsigned off = (in ? l : 0u) * 4u;   // clamped index + select instead of a predicated load
            const float pxx = row_load(row, off, 2 * pl);
            const bool seen = in && !(pxx < 0.0f);   // the update's own first-sighting test: -0 counts as seen
            const bool named = seen && tk[t] < K;
            const u64 mask = __ballot(named);
            const unsigned rank = count + (unsigned)__popcll(mask & below);
            if (named && rank < 64u) {   // (the anchors behind the 64th of a table that names a detection twice take no part)
                s_anchor[0][rank] = row_load(row, off, 0 * pl);
                s_anchor[1][rank] = row_load(row, off, 1 * pl);
                s_anchor[2][rank] = pxx;
                s_anchor[3][rank] = row_load(row, off, 3 * pl);
                s_anchor[4][rank] = row_load(row, off, 4 * pl);
                s_slot[rank] = l;
            }
            count += (unsigned)__popcll(mask);
            nseen += __popcll(__ballot(seen));
        }
    }
    const unsigned A = count < 64u ? count : 64u;
    int nmerged = 0, nrefused = 0;
    if (A != 0u) {   // (wave-uniform)
        wave_lds_sync();
        float w[5];   // lane j: anchor j
#pragma unroll
        for (int p = 0; p < 5; ++p) w[p] = s_anchor[p][lane < A ? lane : 0u];
        const unsigned wslot = s_slot[lane < A ? lane : 0u];
        // 2. the free landmark chooses
        const float inf = __uint_as_float(0x7f800000u);
        for (unsigned b = 0; b < batches; ++b) {
            unsigned tk[2];
            merge_table_bytes<WIDE>(tab, tab_dw, b, lane, L, tk);
            v2f m[5];
            unsigned l[2];
            bool free_[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                l[t] = b * 128u + 64u * t + lane;
                const unsigned off = (l[t] < L ? l[t] : 0u) * 4u;
#pragma unroll
                for (int p = 0; p < 5; ++p) m[p][t] = row_load(row, off, p * pl);
                free_[t] = l[t] < L && !(m[2][t] < 0.0f) && !(tk[t] < K);
            }
            if (__ballot(free_[0] || free_[1]) == 0) continue;   // (wave-uniform) a batch without a free landmark
            v2f mx = m[0];
            const v2f my = m[1], pxx = m[2], pxy = m[3], pyy = m[4];
            // a landmark that takes no part: NaN in its mean makes every m NaN, and NaN passes none of the comparisons below
#pragma unroll
            for (int t = 0; t < 2; ++t) mx[t] = free_[t] ? mx[t] : __uint_as_float(0x7fc00000u);
            v2f best = bc2(inf);
            unsigned bj[2] = { 0u, 0u };
            for (unsigned j = 0; j < A; ++j) {
                const v2f wx = bc2(lane_value(w[0], (int)j)), wy = bc2(lane_value(w[1], (int)j));
                const v2f sa = bc2(lane_value(w[2], (int)j)) + pxx, sb = bc2(lane_value(w[3], (int)j)) + pxy, sc = bc2(lane_value(w[4], (int)j)) + pyy;
                const v2f det = sa * sc - sb * sb;
                const v2f idet = ekf_rcp(det);
                const v2f i00 = sc * idet, i01 = -sb * idet, i11 = sa * idet;
                const v2f dx = mx - wx, dy = my - wy;
                const v2f t0 = i00 * dx + i01 * dy, t1 = i01 * dx + i11 * dy;
                const v2f maha = dx * t0 + dy * t1;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    const bool take = maha[t] < best[t];
                    best[t] = take ? maha[t] : best[t];
                    bj[t] = take ? j : bj[t];
                }
            }
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (free_[t] && best[t] >= 0.0f && best[t] <= a.gate) {
                    const unsigned bits = best[t] == 0.0f ? 0u : __float_as_uint(best[t]);   // -0 -> +0
                    atomicMin(&s_best[bj[t]], ((u64)bits << 32) | l[t]);
                }
        }
        wave_lds_sync();
        // 3. the anchor chooses and absorbs (every lane runs the arithmetic, the stores are selected)
        const u64 won = s_best[lane];
        const bool has = lane < A && won != ~0ull;
        const unsigned lw = has ? (unsigned)won : 0u;   // the absorbed slot (a landmark of this row: it posted itself)
        float f[5], o[5];
#pragma unroll
        for (int p = 0; p < 5; ++p) f[p] = row_load(row, lw * 4u, p * pl);
        merge_fuse(f[0], f[1], f[2], f[3], f[4], w[0], w[1], w[2], w[3], w[4], o);
        const float dpost = o[2] * o[4] - o[3] * o[3];
        const bool fine = merge_finite(o[0]) && merge_finite(o[1]) && merge_finite(o[2]) && merge_finite(o[3]) && merge_finite(o[4]) &&
                          o[2] > 0.0f && o[4] > 0.0f && dpost > 0.0f;
        const bool ok = has && fine;
        if (ok) {
#pragma unroll
            for (int p = 0; p < 5; ++p) row_store(row, wslot * 4u, p * pl, o[p]);
            row_store(row, lw * 4u, 0 * pl, 0.0f);   // the five planes of a slot that was never used
            row_store(row, lw * 4u, 1 * pl, 0.0f);
            row_store(row, lw * 4u, 2 * pl, -1.0f);
            row_store(row, lw * 4u, 3 * pl, 0.0f);
            row_store(row, lw * 4u, 4 * pl, 0.0f);
            if (a.ev) {
                guchar* c = (guchar*)(uniform_gptr(a.ev + (size_t)i * (size_t)a.ev_stride));
                const unsigned sum = (unsigned)c[wslot] + (unsigned)c[lw];   // integers: 200 + 255 does not wrap
                c[wslot] = (uint8_t)(sum < (unsigned)a.cmax ? sum : (unsigned)a.cmax);
                c[lw] = 0;
            }
        }
        nmerged = __popcll(__ballot(ok));
        nrefused = __popcll(__ballot(has && !fine));
    }
    if (lane == 0 && a.stats) {
        int32_t* st3 = a.stats + 3 * (size_t)i;
        st3[0] = nmerged;
        st3[1] = nrefused;
        st3[2] = nseen - nmerged;
    }
}

}  // namespace

bool merge_args_ok(const MergeArgs& a)
{
    return !(a.nlandmarks < 0 || a.nlandmarks > SLAM_MAX_OBS || a.ndet < 0 || a.ndet > SLAM_MAX_DETECTIONS || a.assoc_stride < a.nlandmarks ||
             a.plane_stride < a.nlandmarks || a.row_stride < 5 * (int64_t)a.plane_stride || !(a.gate > 0.0f && a.gate <= 3.402823466e+38f) ||
             !a.map || !a.assoc || (a.ev && (a.ev_stride < a.nlandmarks || a.cmax < 1 || a.cmax > 255)));
}

hipError_t launch_landmark_merge(hipStream_t stream, const MergeArgs& a_in, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (!merge_args_ok(a_in)) return hipErrorInvalidValue;   // what the row, byte and LDS accesses are sized by
    MergeArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (dword_rows(a.assoc, a.assoc_stride)) merge_kernel<true><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else merge_kernel<false><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
