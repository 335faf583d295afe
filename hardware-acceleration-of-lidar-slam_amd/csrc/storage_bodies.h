// Device bodies that the map-storage kernels of more than one unit run, each written once: the ordered compaction of the
// observation table (build_obs_list_kernel of ekf_sparse_kernels.hip and page_list_kernel of paged_kernels.hip feed the same
// list-form updates, so their lists must agree bit for bit) and a migrated record's covariances as a class of its own
// (the unpackers of split_kernels.hip and paged_kernels.hip).
// No counterpart in the reference (it has no particles or landmarks).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ekf_math.h"
#include "kernels.h"

namespace slam {

// ---- One 1024-landmark step of the compaction, one workgroup of 1024 threads, thread t = landmark l = l0 + t.
// In front of the step's first barrier: m = the wavefront's ballot of "observed" -> its count and its 64 bits of the bitmap
// (bits == nullptr: no list wanted, the count alone).
__device__ __forceinline__ void obs_list_mark(unsigned long long m, int l0, int* __restrict__ wave_obs, unsigned* __restrict__ bits)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_obs[wave] = __popcll(m);
    if (bits && lane == 0) bits[(l0 >> 5) + 2 * wave] = (unsigned)m;
    if (bits && lane == 32) bits[(l0 >> 5) + 2 * wave + 1] = (unsigned)(m >> 32);
}

// Behind that barrier: the observation of landmark l (ob; measurement vx, vy) goes to its place in the list — `base`
// observations in the steps before, wave_obs[w] in wavefront w of this one — with its accumulator round; *max_round (LDS)
// keeps the highest round.  ol.id == nullptr: no list.  Returns the list position of this wavefront's first observation.
__device__ __forceinline__ int obs_list_step(unsigned long long m, bool ob, int l, float vx, float vy, const int* __restrict__ wave_obs,
                                             int base, const unsigned* __restrict__ bits, const ObsListOut& ol, int* max_round)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int off = base;
    for (int w = 0; w < wave; ++w) off += wave_obs[w];
    if (ol.id && ob) {
        const int k = off + __popcll(m & ((1ull << lane) - 1ull));
        ol.id[k] = l;
        ol.zx[k] = vx;
        ol.zy[k] = vy;
        // round: earlier observed landmarks with the same l mod 128 = the same bit of every fourth word below
        int r = 0;
        for (int b = l - 128; b >= 0; b -= 128) r += (int)((bits[b >> 5] >> (b & 31)) & 1u);
        ol.round[k] = r;
        if (r > 0) atomicMax(max_round, r);
    }
    return off;
}

// ---- A received record (pose, then five planes of nlandmarks values) brings its covariances along: they become class c,
// the class of staging row `row` — planes, determinant terms (q = meas_var), stamp, and an entry in the list of classes in
// use.  One workgroup of 256 threads.  Padding columns [nlandmarks, Lp): (1, 0, 1), as split_from_rows_kernel leaves them.
__device__ __forceinline__ void unpack_class(const float* __restrict__ rec, int nlandmarks, float q, int c, int row, const ClassStore& cs)
{
    float* __restrict__ cr = cs.cov + (int64_t)c * 3 * cs.Lp;
    float* __restrict__ xr = cs.covx + (int64_t)c * 2 * cs.Lp;
    for (int l = threadIdx.x; l < cs.Lp; l += 256) {
        const bool in_row = l < nlandmarks;
        const float pxx = in_row ? rec[3 + 2 * nlandmarks + l] : 1.0f, pxy = in_row ? rec[3 + 3 * nlandmarks + l] : 0.0f,
                    pyy = in_row ? rec[3 + 4 * nlandmarks + l] : 1.0f;
        cr[l] = pxx;
        cr[cs.Lp + l] = pxy;
        cr[2 * cs.Lp + l] = pyy;
        float idet = 1.0f, hl = 0.0f;
        if (in_row && !(pxx < 0.0f)) ekf_det_terms<float>(pxx, pxy, pyy, q, idet, hl);
        xr[l] = idet;
        xr[cs.Lp + l] = hl;
    }
    if (threadIdx.x == 0) {
        cs.cls[row] = c;
        cs.cstamp[c] = cs.stamp_now;
        cs.live[atomicAdd(cs.cnt, 1)] = c;
    }
}

}  // namespace slam
