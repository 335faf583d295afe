// evidence_common.h — what the kernels of the existence evidence share (evidence_kernels.hip: the stage, init and gather;
// sight_kernels.hip: the sight table; merge_kernels.hip), the misses of the localise stage (localise_kernels.hip) and the host's
// slam_fov_bound: the visibility test's r2, the diamond angle of a direction, the visibility predicate itself
// (evidence_visibility), and the byte traffic of a batch of 128 landmarks as dwords (WIDE) — see the head of evidence_kernels.hip
// for the access shape.
#pragma once

#include "ekf_wave.h"

namespace slam {

typedef __attribute__((address_space(1))) unsigned int guint;

// r2 of the visibility test: six separately rounded float32 operations (tests/_evidence_spec.py), never contracted
__device__ __forceinline__ float evidence_r2(float mx, float my, float px, float py)
{
#pragma clang fp contract(off)
    const float dx = mx - px;
    const float dy = my - py;
    const float t = dx * dx;
    const float u = dy * dy;
    return t + u;
}

// the DIAMOND ANGLE p in [0, 4] of the sensor-frame point (x, y) (tests/_sight_spec.py: bin_of; tests/_fov_spec.py: diamond):
// false — none (the origin, a point that is not finite; p = 0 then).  One IEEE division, every step rounded once.  (Host too:
// slam_fov_bound.)
__host__ __device__ __forceinline__ bool diamond_angle(float x, float y, float& p)
{
#pragma clang fp contract(off)
    const float ax = fabsf(x), ay = fabsf(y);
    const float s = ax + ay;
    const bool has = s > 0.0f && s <= 3.402823466e+38f;   // (NaN fails both)
    const float q = has ? ay / s : 0.0f;                  // IEEE division (-fno-fast-math)
    const bool nx = x < 0.0f, ny = y < 0.0f;              // -0.0 is not negative
    p = nx ? (ny ? 2.0f + q : 2.0f - q) : (ny ? 4.0f - q : q);
    return has;
}

// the direction bin of a diamond angle: quarter = bins / 4 as a float, a power of two: the product is exact; p == 4 wraps to bin 0
__device__ __forceinline__ unsigned diamond_bin(float p, float quarter, unsigned mask)
{
#pragma clang fp contract(off)
    return (unsigned)(int)(p * quarter) & mask;
}

// lo <= hi: the arc [lo, hi]; lo > hi: the arc that wraps through p = 4 = 0.  A bound itself is in view
__device__ __forceinline__ bool fov_in_view(float p, bool has, float lo, float hi, bool wraps)
{
    const bool ge = p >= lo, le = p <= hi;
    return !has || (wraps ? (ge || le) : (ge && le));
}

// THE VISIBILITY PREDICATE of a pose (tests/_evidence_spec.py, _sight_spec.py, _fov_spec.py), the one copy the evidence stage
// (evidence_kernels.hip) and the misses of the localise stage (localise_kernels.hip) share.  What a wavefront knows of its pose
// and of the frame:
struct EvidenceView {
    float px, py, sn, cs;   // the pose; sn, cs = det_sincosf(theta), read only under fov || sight
    float range2;           // view_range * view_range, one float32 product made on the host
    float lo, hi;           // the arc of the diamond angle (fov)
    bool wraps;             // lo > hi
    const float* tab;       // the sight table, staged in LDS (sight)
    float quarter;          // bins / 4
    unsigned mask;          // bins - 1
    float margin;
};
// N landmarks of every lane (means mx, my; open: the landmark can be due a miss at all — it is seen and, where the caller knows
// already, not hit) -> due = open & r2 <= range2 (a NaN mean is not visible); view: its direction in the sensor frame lies in
// the arc (fov; a direction without a diamond angle is in view); hidden: due & view & behind what the scan hit — the nearest
// return of its bin and the two neighbours is closer than (r - margin)^2 (sight).  fov, sight: compile-time constants or
// wave-uniform values.  EVERY LANE OF THE WAVEFRONT TAKES PART: the rotation, the division and the compares run only in
// wavefronts in which some lane is due, the square root and the three table reads only where some lane is due AND in view; the
// results depend on neither skip
template <int N>
__device__ __forceinline__ void evidence_visibility(const EvidenceView& v, bool fov, bool sight, const float (&mx)[N], const float (&my)[N],
                                                    const bool (&open)[N], bool (&due)[N], bool (&view)[N], bool (&hidden)[N])
{
#pragma clang fp contract(off)
    float r2[N];
    bool some = false;
#pragma unroll
    for (int t = 0; t < N; ++t) {
        r2[t] = evidence_r2(mx[t], my[t], v.px, v.py);
        due[t] = open[t] && r2[t] <= v.range2;
        view[t] = true;
        hidden[t] = false;
        some = some || due[t];
    }
    if ((fov || sight) && __ballot(some)) {
        float p[N];
        bool has[N];
        some = false;
#pragma unroll
        for (int t = 0; t < N; ++t) {
            const float dx = mx[t] - v.px, dy = my[t] - v.py;   // the visibility test's own dx, dy
            const float xa = v.cs * dx, xb = v.sn * dy;
            const float zx = xa - xb;                            // z = R(theta) (w - t)
            const float ya = v.sn * dx, yb = v.cs * dy;
            const float zy = ya + yb;
            has[t] = diamond_angle(zx, zy, p[t]);
            view[t] = fov ? fov_in_view(p[t], has[t], v.lo, v.hi, v.wraps) : true;
            some = some || (due[t] && view[t]);
        }
        if (sight && __ballot(some)) {
#pragma unroll
            for (int t = 0; t < N; ++t) {
                const unsigned j = diamond_bin(p[t], v.quarter, v.mask);
                const float near = fminf(fminf(v.tab[(j - 1u) & v.mask], v.tab[j]), v.tab[(j + 1u) & v.mask]);   // (no NaN in the table)
                const float r = sqrtf(r2[t]);   // correctly rounded (NOT __fsqrt_rn: det_math.h)
                const float g = r - v.margin;
                const float g2 = g * g;
                hidden[t] = due[t] && view[t] && has[t] && g > 0.0f && near < g2;   // a NaN anywhere: not hidden
            }
        }
    }
}

// WIDE: the bytes of landmarks l and l + 64 (l = 128 b + lane) out of w — lanes 0..31 hold the batch's 32 dwords of one byte
// array, lanes 32..63 those of another; second = false / true says which.  (Every lane of the wavefront takes part.)
__device__ __forceinline__ void batch_bytes(unsigned w, unsigned lane, bool second, unsigned& c0, unsigned& c1)
{
    const int from = (int)(lane >> 2) + (second ? 32 : 0);
    const unsigned sh = 8u * (lane & 3u);
    c0 = (__shfl(w, from, 64) >> sh) & 255u;
    c1 = (__shfl(w, from + 16, 64) >> sh) & 255u;
}

// WIDE: the new bytes of landmarks l and l + 64 of every lane -> the 32 dwords of batch b of `row`; dwords from ndw on are not stored
__device__ __forceinline__ void batch_store(guint* row, unsigned b, unsigned lane, unsigned c0, unsigned c1, unsigned ndw)
{
    const unsigned sh = 8u * (lane & 3u);
    unsigned v0 = c0 << sh, v1 = c1 << sh;
    v0 |= __shfl_xor(v0, 1, 64);
    v1 |= __shfl_xor(v1, 1, 64);
    v0 |= __shfl_xor(v0, 2, 64);
    v1 |= __shfl_xor(v1, 2, 64);
    const int from = (int)((lane & 15u) * 4u);
    const unsigned o0 = __shfl(v0, from, 64), o1 = __shfl(v1, from, 64);
    const unsigned d = b * 32u + lane;
    if (lane < 32u && d < ndw) row[d] = (lane & 16u) ? o1 : o0;
}

// the columns [from, stride) of a row of bytes <- 0 (WIDE: from is a multiple of 4 then)
template <bool WIDE> __device__ __forceinline__ void zero_tail(guchar* row, unsigned from, unsigned stride, unsigned lane)
{
    if (WIDE) {
        guint* row32 = (guint*)row;
        for (unsigned d = from / 4u + lane; d < stride / 4u; d += 64u) row32[d] = 0u;
    } else {
        for (unsigned c = from + lane; c < stride; c += 64u) row[c] = 0;
    }
}

// every row of a byte array starts on a dword
inline bool dword_rows(const void* base, int stride) { return (stride & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 3u) == 0; }

// what the row and byte accesses of either form are sized by
inline bool evidence_args_ok(const EvidenceArgs& a)
{
    return !(a.nlandmarks < 0 || a.nlandmarks > SLAM_MAX_OBS || a.ndet < 0 || a.ndet > SLAM_MAX_DETECTIONS || a.assoc_stride < a.nlandmarks ||
             a.ev_stride < a.nlandmarks || a.plane_stride < a.nlandmarks || a.hit < 1 || a.hit > 255 || a.miss < 1 || a.miss > 255 ||
             a.cmax < 1 || a.cmax > 255 || (a.anc && a.ev_in == a.ev_out));
}

}  // namespace slam
