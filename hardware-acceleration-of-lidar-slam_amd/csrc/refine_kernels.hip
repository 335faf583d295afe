// refine_kernels.hip — scan-match refinement of many poses (DESIGN.md §7 "Refinement"): the reference's 3 x 3 x 3 lattice of
// candidate poses (FastMatch, Subsystem_1/main.c:424-563) laid around EVERY pose, scored like score_body.h scores a pose, the
// pose moved to the winner, `sweeps` times.  Two deliberate differences from FastMatch: headings go through det_sincosf (the
// particle path's trig), and the centre is the incumbent — a candidate wins only with a score strictly below the centre's and
// below every candidate before it (theta-major, x, y-minor), so a pose whose 27 candidates tie stays where it is.
//
// What the lattice shares, and how the kernel uses it:
//  - THREE LANES PER POSE, one per heading (21 poses per wavefront, lane 63 idles along with pose 20's first lane).  A lane
//    keeps its heading's 9 sums and 9 counts in registers and walks the beams in order: every candidate's float sum runs in
//    beam order inside one lane, the reference's sequential sum, with no cross-lane traffic in the beam loop.
//  - per beam and heading the rotation ((X c) + (Y s)) is computed once; the three x offsets and three y offsets give three
//    column and three row indices — 6 roundings — and their 9 combinations 9 cells.  Each is the scorer's
//    ((X c) + (Y s)) + off bit for bit: the last add is the only operation that differs between the candidates.
//  - the 9 cells of a beam are neighbours (a 3 x 3 patch `step_xy` apart): on the packed byte grid (16 x 8 cells per line)
//    they fall in one to four lines, and the 9 gathers of a beam are independent — with two beams per step a lane has 18
//    gathers in flight while it decodes and sums the 18 of the step before.
//  - the scorer's exact tricks (score_body.h): trunc(v + copysign(0.5 - 1 ulp)) for (int)roundf(v), the unsigned bounds test,
//    the buffer resource whose range check turns offset 0xffffffff into +0.0f / code 0 for an out-of-bounds beam.
// The arg-min runs once per sweep: the 27 scores and counts go round the three lanes with wavefront shuffles and every lane
// of the pose applies the incumbent rule literally.  A wavefront leaves the sweep loop as soon as the centre won for all of
// its poses (the same lattice would give the same winner again); the others repeat a sweep that cannot change them.
// Compiled with -ffp-contract=off like the scorer.

#include "det_math.h"
#include "kernels.h"

namespace slam {

namespace {

constexpr int kRefineBlock = 256;
constexpr int kRefinePosesPerWave = 21;                                   // 3 lanes each; lane 63 idles
constexpr int kRefinePosesPerBlock = kRefinePosesPerWave * (kRefineBlock / 64);
constexpr int kRefineRound = 2;   // beams per pipeline step (one float2 pair): 18 gathers in flight per lane

typedef float v2f __attribute__((ext_vector_type(2)));
typedef int v2i __attribute__((ext_vector_type(2)));

struct RefineParams {
    float step_xy, step_theta;
    int sweeps;
};

template <bool MOTION, bool PACKED>
__global__ __launch_bounds__(kRefineBlock) void refine_poses_kernel(ScoreGrid g, const float* __restrict__ bx,
                                                                     const float* __restrict__ by, int nbeams, MotionIO mio,
                                                                     int nposes, RefineParams rp, float* __restrict__ score,
                                                                     int32_t* __restrict__ count, MotionParams mpar)
{
    extern __shared__ float4 s_pair[];
    // beams in pairs, pixel-scaled, padded with NaN to a whole pair (at least one): a NaN beam is out of bounds and adds +0
    const int npairs = nbeams > 0 ? (nbeams + kRefineRound - 1) / kRefineRound : 1;
    {
        const float nanv = __builtin_nanf("");
        for (int p = threadIdx.x; p < npairs; p += kRefineBlock) {
            const int b0 = 2 * p, b1 = b0 + 1;
            s_pair[p] = make_float4(b0 < nbeams ? bx[b0] * g.ipix : nanv, b1 < nbeams ? bx[b1] * g.ipix : nanv,
                                    b0 < nbeams ? by[b0] * g.ipix : nanv, b1 < nbeams ? by[b1] * g.ipix : nanv);
        }
    }
    float* s_table = reinterpret_cast<float*>(s_pair + npairs);   // PACKED: the decode table behind the beams (1 KB)
    if constexpr (PACKED) {
        static_assert(kRefineBlock == 256, "one table entry per thread");
        s_table[threadIdx.x] = g.table[threadIdx.x];
    }
    __syncthreads();

    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int tri = lane < 63 ? lane / 3 : kRefinePosesPerWave - 1;   // lane 63 shadows lane 60 (all lanes stay active)
    const int a = lane < 63 ? lane - 3 * tri : 0;                    // this lane's heading: theta - r, theta, theta + r
    const int base = 3 * tri;                                        // the pose's first lane
    const int pose = ((int)blockIdx.x * (kRefineBlock / 64) + wave) * kRefinePosesPerWave + tri;
    const int i = pose < nposes ? pose : nposes - 1;                 // whole wavefronts stay active for the shuffles
    const bool writer = lane == base && pose < nposes;

    float x, y, th;
    if constexpr (MOTION) {
        const int j = mio.anc ? mio.anc[i] : i;
        motion_sample_one(mpar, (uint64_t)i, mio.sx[j], mio.sy[j], mio.sth[j], x, y, th);
    } else {
        x = mio.x[i];
        y = mio.y[i];
        th = mio.th[i];
    }

    // the scorer's bounds test: 1 <= c <= n - 2 on the rounded cell c as (unsigned)(c - 1) < n - 2 (score_body.h)
    const unsigned lim_x = (unsigned)(g.cols > 2 ? g.cols - 2 : 0);
    const unsigned lim_y = (unsigned)(g.rows > 2 ? g.rows - 2 : 0);
    const unsigned ld4 = (unsigned)g.ld * 4u;          // < 2^24 (the engine refuses wider grids): 24-bit multiply
    const unsigned strip = (unsigned)g.strip_bytes;   // PACKED: bytes of one 16-column strip (< 2^24)
    const __amdgpu_buffer_rsrc_t edt =
        PACKED ? __builtin_amdgcn_make_buffer_rsrc((void*)g.packed, 0, (int)(((unsigned)g.cols + 15u) / 16u * strip), 0x00020000)
               : __builtin_amdgcn_make_buffer_rsrc((void*)g.edt, 0, (int)((unsigned)g.rows * ld4), 0x00020000);
    const v2i sign2 = {(int)0x80000000, (int)0x80000000}, half2 = {0x3effffff, 0x3effffff};   // 0.5 - 1 ulp

    float best = 0.0f;
    int best_n = 0;
    for (int sweep = 0; sweep < rp.sweeps; ++sweep) {
        // the lattice around (x, y, th), laid out as FastMatch lays it out: one binary32 subtract or add each
        const float xs[3] = {x - rp.step_xy, x, x + rp.step_xy};
        const float ys[3] = {y - rp.step_xy, y, y + rp.step_xy};
        const float ths[3] = {th - rp.step_theta, th, th + rp.step_theta};
        float st, ct;
        det_sincosf(a == 0 ? ths[0] : (a == 1 ? ths[1] : ths[2]), st, ct);
        const float nst = -st;
        const v2f c2 = {ct, ct}, s2 = {st, st}, ns2 = {nst, nst};
        v2f ox[3], oy[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float fx = (xs[k] - g.min_x) * g.ipix, fy = (ys[k] - g.min_y) * g.ipix;
            ox[k] = (v2f){fx, fx};
            oy[k] = (v2f){fy, fy};
        }
        float acc[9];
        int cnt[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            acc[k] = 0.0f;
            cnt[k] = 0;
        }
        // beams 2m and 2m + 1 against the heading's 9 candidates (k = 3 * ix + iy): h[2k + e] = the cell's float (PACKED: its code)
        auto gather = [&](int m, float* h) {
            const float4 q = s_pair[m];
            const v2f X = {q.x, q.y}, Y = {q.z, q.w};
            const v2f rx = (X * c2) + (Y * s2);
            const v2f ry = (X * ns2) + (Y * c2);
            unsigned col[3][2], row[3][2];
            bool inx[3][2], iny[3][2];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v2f fx = rx + ox[k];
                v2f fy = ry + oy[k];
                // (int)roundf(f) as trunc(f + copysign(0.5 - 1 ulp, f)), exact for every float (tests/test_oracle_pf.py)
                fx = fx + __builtin_bit_cast(v2f, (__builtin_bit_cast(v2i, fx) & sign2) | half2);
                fy = fy + __builtin_bit_cast(v2f, (__builtin_bit_cast(v2i, fy) & sign2) | half2);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    int ix, iy;   // truncates, saturates and maps NaN to 0
                    asm("v_cvt_i32_f32 %0, %1" : "=v"(ix) : "v"(fx[e]));
                    asm("v_cvt_i32_f32 %0, %1" : "=v"(iy) : "v"(fy[e]));
                    inx[k][e] = (unsigned)(ix - 1) < lim_x;
                    iny[k][e] = (unsigned)(iy - 1) < lim_y;
                    if constexpr (PACKED) {
                        col[k][e] = __umul24((unsigned)ix >> 4, strip) + ((unsigned)ix & 15u);
                        row[k][e] = (unsigned)iy << 4;
                    } else {
                        col[k][e] = (unsigned)ix << 2;
                        row[k][e] = __umul24((unsigned)iy, ld4);
                    }
                }
            }
#pragma unroll
            for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const bool in = inx[kx][e] && iny[ky][e];
                        const unsigned off = in ? col[kx][e] + row[ky][e] : 0xffffffffu;   // out of range: +0.0f / code 0
                        if constexpr (PACKED)
                            h[2 * (3 * kx + ky) + e] = __uint_as_float((unsigned)__builtin_amdgcn_raw_buffer_load_b8(edt, (int)off, 0, 0));
                        else
                            h[2 * (3 * kx + ky) + e] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(edt, (int)off, 0, 0));
                        cnt[3 * kx + ky] += in ? 1 : 0;
                    }
        };
        auto sum = [&](const float* h) {   // the step's two beams in order, per candidate
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                float h0 = h[2 * k], h1 = h[2 * k + 1];
                if constexpr (PACKED) {
                    h0 = s_table[__float_as_uint(h0)];
                    h1 = s_table[__float_as_uint(h1)];
                }
                acc[k] = acc[k] + h0;
                acc[k] = acc[k] + h1;
            }
        };
        float hq[18], hn[18];
        gather(0, hq);
        for (int m = 1; m < npairs; ++m) {
            gather(m, hn);
            sum(hq);
#pragma unroll
            for (int k = 0; k < 18; ++k) hq[k] = hn[k];
        }
        sum(hq);

        // the incumbent rule, literally, in every lane of the pose: the centre first, then the 27 candidates in the reference's order
        best = __shfl(acc[4], base + 1);
        best_n = __shfl(cnt[4], base + 1);
        int win = 13;
#pragma unroll
        for (int h = 0; h < 3; ++h)
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                const float v = __shfl(acc[k], base + h);
                const int vn = __shfl(cnt[k], base + h);
                if (v < best) {
                    best = v;
                    best_n = vn;
                    win = 9 * h + k;
                }
            }
        const int wa = win / 9, wx = (win / 3) % 3, wy = win % 3;
        th = wa == 0 ? ths[0] : (wa == 1 ? ths[1] : ths[2]);
        x = wx == 0 ? xs[0] : (wx == 1 ? xs[1] : xs[2]);
        y = wy == 0 ? ys[0] : (wy == 1 ? ys[1] : ys[2]);
        if (__all(win == 13)) break;   // every pose of the wavefront is a fixed point of its lattice
    }
    if (writer) {
        mio.x[i] = x;
        mio.y[i] = y;
        mio.th[i] = th;
        score[i] = best;
        count[i] = best_n;
    }
}

}  // namespace

namespace {
hipError_t launch_refine_any(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams, const MotionIO& io,
                             int nposes, float step_xy, float step_theta, int sweeps, const MotionParams* motion, float* score,
                             int32_t* count, const EventPair* ev)
{
    if (nposes <= 0) return hipSuccess;
    const int blocks = (nposes + kRefinePosesPerBlock - 1) / kRefinePosesPerBlock;
    const bool packed = g.packed != nullptr;   // the byte-per-cell copy of the grid + 1 KB of LDS for its table
    const int npairs = nbeams > 0 ? (nbeams + kRefineRound - 1) / kRefineRound : 1;
    const size_t lds = sizeof(float4) * (size_t)npairs + (packed ? 1024 : 0);
    const RefineParams rp{ step_xy, step_theta, sweeps };
    if (ev) (void)hipEventRecord(ev->start, stream);
#define SLAM_LAUNCH_REFINE(MOTION, PK)                                                                                       \
    refine_poses_kernel<MOTION, PK><<<blocks, kRefineBlock, lds, stream>>>(g, bx, by, nbeams, io, nposes, rp, score, count, \
                                                                          motion ? *motion : MotionParams{})
    if (motion) {
        if (packed) SLAM_LAUNCH_REFINE(true, true); else SLAM_LAUNCH_REFINE(true, false);
    } else {
        if (packed) SLAM_LAUNCH_REFINE(false, true); else SLAM_LAUNCH_REFINE(false, false);
    }
#undef SLAM_LAUNCH_REFINE
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}
}  // namespace

hipError_t launch_refine_poses(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams, float* x, float* y,
                               float* th, int nposes, float step_xy, float step_theta, int sweeps, float* score, int32_t* count,
                               const EventPair* ev)
{
    const MotionIO io{ nullptr, nullptr, nullptr, nullptr, x, y, th, FreeListRider() };
    return launch_refine_any(stream, g, bx, by, nbeams, io, nposes, step_xy, step_theta, sweeps, nullptr, score, count, ev);
}

hipError_t launch_motion_refine(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams, const MotionIO& io,
                                int nposes, int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame,
                                float step_xy, float step_theta, int sweeps, float* score, int32_t* count, const EventPair* ev)
{
    const MotionParams mpar = make_motion_params(first_id, dp, sigma, seed, frame);
    return launch_refine_any(stream, g, bx, by, nbeams, io, nposes, step_xy, step_theta, sweeps, &mpar, score, count, ev);
}

}  // namespace slam
