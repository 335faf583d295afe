// evidence_common.h — what the kernels of the existence evidence share (evidence_kernels.hip: the stage, init and gather;
// sight_kernels.hip: the sight table; merge_kernels.hip) and the host's slam_fov_bound: the visibility test's r2, the diamond
// angle of a direction, and the byte traffic of a batch of 128 landmarks as dwords (WIDE) — see the head of evidence_kernels.hip
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
