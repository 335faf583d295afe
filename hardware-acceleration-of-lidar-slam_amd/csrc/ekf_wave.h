// ekf_wave.h — what every form of the landmark update (the 2x2 EKF per (particle, landmark)) shares: row
// access through wave-uniform descriptors, the log-likelihood's sum and store, the workgroup renumbering and its grid, a
// particle's pose and a group's accumulators in LDS.  The forms: ekf_row_body.h (a row per
// wavefront), ekf_group_body.h (grouped), ekf_split_body.h (split layout), front_kernels.hip (fused with the scorer into the
// front of a frame), ekf_sparse_kernels.hip (sparse in place behind the compact observation list).
// None of these stages exists in the reference: the specification is DESIGN.md
// + oracle/slam_oracle_pf.c, and these kernels match that specification bit for bit.
//
// Data layout (HBM): particles are SoA float arrays; the landmark maps are ONE ROW PER PARTICLE,
// [particle][5 planes: mu_x, mu_y, P_xx, P_xy, P_yy][plane_stride floats], so that a wavefront walking one
// particle's landmarks moves 256 contiguous bytes per plane and access, and the offspring of one resample
// ancestor (neighbouring particles) share its row through L2.
// All kernels are HBM-streaming or latency-bound integer work; there is no GEMM shape here
// (the largest matrix is 2x2), hence no MFMA.
#pragma once

#include "det_math.h"
#include "ekf_math.h"
#include "pf_common.h"

namespace slam {

__device__ __forceinline__ float wave_xor_tree_sum(float v)   // t[j] = t[j] + t[j ^ s], s = 1 .. 32: all lanes equal
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

// wave_xor_tree_sum of G values per lane (the sums of a group's G particles) without doing every addition twice.  In a step
// of the butterfly lanes j and j ^ s add the same two values; here, while a lane still holds more than one particle, the
// two share the work: of each pair of neighbouring values lane j keeps the one whose particle has the bit of s as j has it and
// hands the other to lane j ^ s, which keeps exactly that one.  After log2 G steps a lane holds ONE particle, j & (G - 1),
// and the remaining steps run on it as in the butterfly: G - 1 + 6 - log2 G exchanges and additions instead of 6 G.  What lane
// j adds for the particle it ends up with is, step by step, what the butterfly adds in lane j for that particle — own value
// first, the partner's second —, so the value returned in lane j is the butterfly's t[j & (G - 1)] of lane j bit for bit: lane
// k < G holds particle k's total (tests/test_reduce_schedule_cpu.py walks the schedule lane by lane).
template <int G>
__device__ __forceinline__ float wave_halving_tree_sums(const float (&t)[G], unsigned lane)
{
    static_assert(G == 2 || G == 4 || G == 8, "a power of two below the wavefront's size");
    float v[G];
#pragma unroll
    for (int k = 0; k < G; ++k) v[k] = t[k];
    int s = 1;
#pragma unroll
    for (int m = G; m > 1; m >>= 1, s <<= 1) {
        const bool up = (lane & (unsigned)s) != 0;
#pragma unroll
        for (int i = 0; i < m / 2; ++i) {
            const float keep = up ? v[2 * i + 1] : v[2 * i];
            const float send = up ? v[2 * i] : v[2 * i + 1];
            v[i] = keep + __shfl_xor(send, s, 64);
        }
    }
#pragma unroll
    for (; s < 64; s <<= 1) v[0] = v[0] + __shfl_xor(v[0], s, 64);
    return v[0];
}

constexpr int kEkfWaves = 4;   // particles per workgroup

// global-address-space pointers: "scalar base + 32-bit lane offset" is an addressing mode of global_load/store only
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) unsigned char guchar;
// cache policy of the row stores: 2 = nt (streaming; the written rows are next read a frame later, long after they
// left the caches).  Measured at 64k x 500: default 170 us, nt 162 us, sc0 170 us, sc1 171 us in the filter;
// 243 / 248 / 244 / 243 us for a sweep without shared ancestors.
constexpr int kEkfStoreAux = 2;
__device__ __forceinline__ float row_load(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff)
{
    return __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, (int)voff, soff, 0));
}
__device__ __forceinline__ void row_store(__amdgpu_buffer_rsrc_t r, unsigned voff, int soff, float v)
{
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), r, (int)voff, soff, kEkfStoreAux);
}
__device__ __forceinline__ gchar* uniform_gptr(const void* p)   // tell the compiler the pointer is wave-uniform
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return (gchar*)(((uint64_t)hi << 32) | lo);
}
// `bytes` of row `row` (rows `stride` floats apart) as a buffer resource: a wave-uniform descriptor in SGPRs
__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float* base, int row, int64_t stride, int bytes)
{
    return __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(base + (int64_t)row * stride), 0, bytes, 0x00020000);
}

// Workgroups are dealt to the 8 XCDs round-robin.  Renumber them so that each XCD (one L2) works on one
// contiguous eighth of the particles: the offspring of an ancestor then share ONE L2 instead of up to eight.
__device__ __forceinline__ int xcd_block(int chunk)   // chunk: workgroups per XCD (gridDim.x == 8 * chunk), 0: as dealt
{
    const int bid = blockIdx.x;
    return chunk > 0 ? (bid & 7) * chunk + (bid >> 3) : bid;
}
// The grid of a launch whose workgroups own `per_block` particles each, XCD-contiguous numbering (xcd_block) from 64
// workgroups on: the grid is padded to a multiple of 8 (surplus workgroups exit at once) and xcd_chunk = workgroups per XCD;
// smaller grids stay as they are, xcd_chunk = 0.
inline int xcd_grid(int n, int per_block, int& xcd_chunk)
{
    const int blocks = (n + per_block - 1) / per_block;
    xcd_chunk = blocks >= 64 ? (blocks + 7) / 8 : 0;
    return xcd_chunk ? 8 * xcd_chunk : blocks;
}

__device__ __forceinline__ void store_loglik(const EkfArgs& a, int i, float total)   // particle i's log-likelihood
{
    a.loglik[i] = total;
    if (a.loglik_user) a.loglik_user[i] = total;
}

__device__ __forceinline__ float lane_value(float v, int k)   // lane k's value, wave-uniform (v_readlane_b32)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), k));
}

struct EkfPose {   // one particle of the group (wave-uniform values)
    __amdgpu_buffer_rsrc_t rout;
    v2f s, c, px, py;
};

// the accumulator pair of particle k of a wavefront's group in LDS (s_acc: per particle the 128 accumulators of the specification)
template <int G>
__device__ __forceinline__ v2f acc_load(float (*s_acc)[G][128], int wave, int k, unsigned lane)
{
    return (v2f){s_acc[wave][k][lane], s_acc[wave][k][lane + 64]};
}
template <int G>
__device__ __forceinline__ void acc_store(float (*s_acc)[G][128], int wave, int k, unsigned lane, v2f acc)
{
    s_acc[wave][k][lane] = acc[0];
    s_acc[wave][k][lane + 64] = acc[1];
}

}  // namespace slam
