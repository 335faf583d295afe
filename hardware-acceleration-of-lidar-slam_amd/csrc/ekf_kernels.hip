// ekf_kernels.hip — the motion sample and the landmark update of the particle filter: the 2x2 EKF
// per (particle, landmark) in every form — a row per wavefront, grouped, on the split layout, fused with the scorer into the
// front of a frame, sparse in place behind the compact observation list — plus the copy ceiling and the reciprocal self-test.
// None of these stages exists in the reference: the specification is DESIGN.md
// + oracle/slam_oracle_pf.c, and these kernels match that specification bit for bit.  The only
// reference anchor is the zero-noise motion step = the constant-velocity predict of
// Subsystem_1/main.c:875-898.
//
// Data layout (HBM): particles are SoA float arrays; the landmark maps are ONE ROW PER PARTICLE,
// [particle][5 planes: mu_x, mu_y, P_xx, P_xy, P_yy][plane_stride floats], so that a wavefront walking one
// particle's landmarks moves 256 contiguous bytes per plane and access, and the offspring of one resample
// ancestor (neighbouring particles) share its row through L2.
// All kernels are HBM-streaming or latency-bound integer work; there is no GEMM shape here
// (the largest matrix is 2x2), hence no MFMA.

#include "det_math.h"
#include "ekf_math.h"
#include "score_body.h"
#include "pf_common.h"
#include "storage_bodies.h"

namespace slam {

namespace {

// ------------------------------------------------------------------ A9: motion sample
__global__ __launch_bounds__(kBlock) void motion_sample_kernel(const float* __restrict__ sx,
                                                               const float* __restrict__ sy,
                                                               const float* __restrict__ sth,
                                                               const int32_t* __restrict__ anc, float* __restrict__ x,
                                                               float* __restrict__ y, float* __restrict__ th, int n,
                                                               MotionParams mp)
{
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int j = anc ? anc[i] : i;
    float ox, oy, ot;
    motion_sample_one(mp, (uint64_t)i, sx[j], sy[j], sth[j], ox, oy, ot);
    x[i] = ox;
    y[i] = oy;
    th[i] = ot;
}

// ------------------------------------------------------------------ A10: 2x2 EKF per (particle, landmark)
// The map is one row per particle (5 planes of plane_stride floats).  ONE WAVEFRONT OWNS ONE PARTICLE and its
// lanes walk the landmarks of the row, two landmarks per lane (l and l + 64 of each batch of 128), so that every
// load and store is a coalesced 256-byte access and the arithmetic runs on float2 (v_pk_mul_f32 / v_pk_add_f32:
// IEEE per component, i.e. the same bits as the scalar form).  The observations of the frame come as a table indexed by
// landmark (zx[l], zy[l], NaN = not observed), read alongside the row.  Why rows: after a resample most
// particles are copies of few ancestors (the bench's filter keeps ~6 % distinct), the offspring of one ancestor
// are neighbouring particles, so the 10 KB source row is fetched from HBM once and re-read from L2 by the other
// offspring — the sweep's HBM traffic is the 20 B/(particle, landmark) it writes plus the distinct rows it reads,
// not 40 B.  Row base addresses are wave-uniform (SGPR).
__device__ __forceinline__ float wave_xor_tree_sum(float v)   // t[j] = t[j] + t[j ^ s], s = 1 .. 32: all lanes equal
{
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

constexpr int kEkfWaves = 4;   // particles per workgroup

// global-address-space pointers: "scalar base + 32-bit lane offset" is an addressing mode of global_load/store only
typedef __attribute__((address_space(1))) char gchar;
typedef __attribute__((address_space(1))) float gfloat;
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

struct EkfLane {   // per-wavefront constants of one particle
    // source row and destination row as buffer resources (wave-uniform descriptors in SGPRs): an access is
    // "descriptor + 32-bit lane offset + scalar plane offset", no 64-bit vector arithmetic for loads or stores
    __amdgpu_buffer_rsrc_t rin, rout;
    int pl;   // plane stride in bytes
    const gchar *ozx, *ozy;
    unsigned L;
    v2f s, c, px, py, q;
};

// What goes into the row for the two landmarks of a lane, given the update's result in r0 .. r4 / ll: a first sighting
// (prior P_xx < 0) takes the observed point and P = q I and adds no likelihood term; a landmark without an observation keeps
// its prior values.  Both cases are decided for the WAVEFRONT first (a ballot each): in a running filter most batches of
// 128 landmarks hold neither — every landmark seen before, every one observed, or none — and then the selects (and the
// arithmetic of the first sighting) are skipped altogether.  The values are those of
//     ob ? (first ? {f0, f1, q, 0, q; 0} : {o0 .. o4; ll}) : {prior; 0}
// in every case.
__device__ __forceinline__ void ekf_select(v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll, v2f mx, v2f my, v2f pxx, v2f pxy,
                                           v2f pyy, v2f zx, v2f zy, v2f s, v2f c, v2f px, v2f py, v2f q, bool ob0, bool ob1)
{
    if (__ballot(pxx[0] < 0.0f || pxx[1] < 0.0f) != 0) {
        v2f f0, f1;
        ekf_first_sighting<v2f>(zx, zy, s, c, px, py, f0, f1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool first = pxx[t] < 0.0f;
            r0[t] = first ? f0[t] : r0[t];
            r1[t] = first ? f1[t] : r1[t];
            r2[t] = first ? q[t] : r2[t];
            r3[t] = first ? 0.0f : r3[t];
            r4[t] = first ? q[t] : r4[t];
            ll[t] = first ? 0.0f : ll[t];
        }
    }
    if (__ballot(!(ob0 && ob1)) != 0) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool ob = t ? ob1 : ob0;
            r0[t] = ob ? r0[t] : mx[t];
            r1[t] = ob ? r1[t] : my[t];
            r2[t] = ob ? r2[t] : pxx[t];
            r3[t] = ob ? r3[t] : pxy[t];
            r4[t] = ob ? r4[t] : pyy[t];
            ll[t] = ob ? ll[t] : 0.0f;
        }
    }
}

// NB batches of 128 landmarks starting at lb: all loads first, then the arithmetic, then the stores.  A lane owns
// landmarks l and l + 64 of each batch, so every access is one 256-byte dword access per wavefront (8-byte
// accesses, a lane owning neighbours, were measured ~20 % slower whenever the source rows come out of L2).
// FULL: every lane's landmarks lie inside the row (lb + 128*NB <= plane_stride) and the update is out of place,
// so nothing is predicated; landmarks at or beyond L (row padding) then simply count as "not observed" and their
// padding values are copied along.  !FULL: the general form (row tails, in-place updates).
template <int NB, bool FULL, bool COPY>
__device__ __forceinline__ void ekf_batches(const EkfLane& w, unsigned lb, unsigned lane, v2f& acc)
{
    const float nan = __uint_as_float(0x7fc00000u);
    v2f m[NB][5], zx[NB], zy[NB];
    unsigned off[NB][2];
    bool obs[NB][2], use[NB][2];
#pragma unroll
    for (int g = 0; g < NB; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = lb + (unsigned)g * 128u + 64u * t + lane;
            const bool in = l < w.L;
            off[g][t] = ((FULL || in) ? l : 0u) * 4u;
            const unsigned zo = (in ? l : 0u) * 4u;   // clamped index + select instead of a predicated load
            const float vx = *(const gfloat*)(w.ozx + zo), vy = *(const gfloat*)(w.ozy + zo);
            zx[g][t] = in ? vx : nan;
            zy[g][t] = in ? vy : nan;
            // NaN = no observation (also what lanes beyond L were given).  Testing zy as well keeps its load up here
            // with the others: the compiler otherwise sinks it into the arithmetic, two extra round trips per batch.
            obs[g][t] = zx[g][t] == zx[g][t] && zy[g][t] == zy[g][t];
            use[g][t] = FULL ? true : (COPY ? in : obs[g][t]);
        }
#pragma unroll
    for (int g = 0; g < NB; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (FULL || use[g][t]) {
#pragma unroll
                for (int p = 0; p < 5; ++p) m[g][p][t] = row_load(w.rin, off[g][t], p * w.pl);
            }
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        if (!FULL && !(use[g][0] || use[g][1])) continue;
        const v2f mx = m[g][0], my = m[g][1], pxx = m[g][2], pxy = m[g][3], pyy = m[g][4];
        if (COPY && __ballot(obs[g][0] || obs[g][1]) == 0) {   // no observation among these 128 landmarks: plain copy
#pragma unroll
            for (int t = 0; t < 2; ++t)
                if (FULL || use[g][t]) {
#pragma unroll
                    for (int p = 0; p < 5; ++p) row_store(w.rout, off[g][t], p * w.pl, m[g][p][t]);
                }
            continue;
        }
        const v2f q = w.q;
        const EkfResult<v2f> u = ekf_update_one<v2f, false>(mx, my, pxx, pxy, pyy, zx[g], zy[g], w.s, w.c, w.px, w.py, q);
        v2f r0 = u.o0, r1 = u.o1, r2 = u.o2, r3 = u.o3, r4 = u.o4, ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx[g], zy[g], w.s, w.c, w.px, w.py, q, obs[g][0], obs[g][1]);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (FULL || use[g][t]) {
                row_store(w.rout, off[g][t], 0 * w.pl, r0[t]);
                row_store(w.rout, off[g][t], 1 * w.pl, r1[t]);
                row_store(w.rout, off[g][t], 2 * w.pl, r2[t]);
                row_store(w.rout, off[g][t], 3 * w.pl, r3[t]);
                row_store(w.rout, off[g][t], 4 * w.pl, r4[t]);
            }
        acc = acc + ll;
    }
}

// NB: batches of 128 landmarks per pass of the fast path.  COPY: out of place.
template <int NB, bool COPY>
__global__ __launch_bounds__(kEkfWaves * 64) void ekf_update_kernel(EkfArgs a)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    // Workgroups are dealt to the 8 XCDs round-robin.  Renumber them so that each XCD (one L2) works on one
    // contiguous eighth of the particles: the offspring of an ancestor then share ONE L2 instead of up to eight.
    int bid = blockIdx.x;
    if (a.xcd_chunk > 0) {
        const int per = a.xcd_chunk;   // workgroups per XCD, gridDim.x == 8 * per
        bid = (bid & 7) * per + (bid >> 3);
    }
    const int i = bid * kEkfWaves + wave;
    if (i >= a.n) return;
    const int src = a.anc ? a.anc[i] : i;
    float st_, ct_;
    det_sincosf(a.th[i], st_, ct_);
    EkfLane w;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    w.rin = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_in + (int64_t)src * a.row_stride), 0, row_bytes, 0x00020000);
    w.rout = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_out + (int64_t)i * a.row_stride), 0, row_bytes, 0x00020000);
    w.pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    w.ozx = uniform_gptr(a.obs_zx);
    w.ozy = uniform_gptr(a.obs_zy);
    w.L = (unsigned)a.nlandmarks;
    w.s = bc2(st_); w.c = bc2(ct_); w.px = bc2(a.x[i]); w.py = bc2(a.y[i]); w.q = bc2(a.meas_var);

    v2f acc = bc2(0.0f);   // lane j: .x = accumulator j, .y = accumulator j + 64 of the spec (landmark l -> l mod 128)
    unsigned lb = 0;
    if (COPY) {   // whole batches that fit into the row, padding included: nothing predicated
        const unsigned room = (unsigned)a.plane_stride;
        for (; lb < w.L && lb + 128u * NB <= room; lb += 128u * NB) ekf_batches<NB, true, COPY>(w, lb, lane, acc);
        if (NB > 1)
            for (; lb < w.L && lb + 128u <= room; lb += 128u) ekf_batches<1, true, COPY>(w, lb, lane, acc);
    }
    // the general form (row tails; in-place updates).  In place only observed landmarks are touched, so a wavefront's
    // time is round trips, not bytes: NB batches go through one round trip together (batches beyond L load nothing).
    constexpr int NBT = COPY ? 1 : NB;
    for (; lb < w.L; lb += 128u * NBT) ekf_batches<NBT, false, COPY>(w, lb, lane, acc);

    const float total = wave_xor_tree_sum(acc[0] + acc[1]);
    if (lane == 0) {
        a.loglik[i] = total;
        if (a.loglik_user) a.loglik_user[i] = total;
    }
}

// ---- grouped form of the out-of-place update: ONE WAVEFRONT OWNS G NEIGHBOURING PARTICLES (G = 2, 4 or 8).
// After a resample the slots are sorted by ancestor, so neighbouring particles mostly descend from the same one.  The
// row-per-wavefront kernel lets them share the source row through L2; measured (profiles/copy_ceiling.hip) even a pure copy
// pays for that — 155 us at 64k x 512 columns when 16 neighbours share a source, against 109 us when nothing is re-read.
// Here the wavefront walks the landmarks in the OUTER loop and its G particles in the inner one: a batch of the source
// row stays in registers while every particle of the group that descends from it is updated with its own pose and stored
// to its own row — the re-reads never leave the register file, the observation table is read once per group.  Per
// (particle, landmark) the arithmetic, its order and the log-likelihood summation are those of ekf_batches (bit-exact:
// the same tests cover both kernels); the per-particle accumulators live in LDS between batches.
template <int NB>
struct EkfBatch {   // NB batches of 128 landmarks of one source row + the observations of those landmarks
    v2f mx[NB], my[NB];        // prior means
    v2f p2[NB], p3[NB], p4[NB];   // what goes into the covariance planes: (I - W) P, q I for a first sighting, the prior without an observation
    EkfShared<v2f> sh[NB];     // the pose-independent part of the update (csrc/ekf_math.h), worked out once per source row
    v2f zx[NB], zy[NB];
    bool obs[NB][2], first[NB][2];
    bool any_obs[NB], all_obs[NB], any_first[NB];   // wave-uniform
    unsigned off[NB][2];
};

struct EkfPose {   // one particle of the group (wave-uniform values)
    __amdgpu_buffer_rsrc_t rout;
    v2f s, c, px, py;
};

// A new source row is in registers (b.mx / b.my and the prior covariance pxx / pxy / pyy of batch g): everything about it
// that does not depend on the particle — the gain, the posterior covariance, the determinant's logarithm (ekf_shared) and
// the selection of what the covariance planes receive (a first sighting: q I; no observation: the prior).
template <int NB>
__device__ __forceinline__ void ekf_prepare(EkfBatch<NB>& b, int g, v2f pxx, v2f pxy, v2f pyy, v2f q)
{
    b.p2[g] = pxx;
    b.p3[g] = pxy;
    b.p4[g] = pyy;
    b.first[g][0] = pxx[0] < 0.0f;
    b.first[g][1] = pxx[1] < 0.0f;
    b.any_first[g] = __ballot(b.first[g][0] || b.first[g][1]) != 0;
    if (!b.any_obs[g]) return;   // no observation among these 128 landmarks: the rows are copied
    b.sh[g] = ekf_shared<v2f>(pxx, pxy, pyy, q);
    v2f r2 = b.sh[g].o2, r3 = b.sh[g].o3, r4 = b.sh[g].o4;
    if (b.any_first[g]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            r2[t] = b.first[g][t] ? q[t] : r2[t];
            r3[t] = b.first[g][t] ? 0.0f : r3[t];
            r4[t] = b.first[g][t] ? q[t] : r4[t];
        }
    }
    if (!b.all_obs[g]) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            r2[t] = b.obs[g][t] ? r2[t] : pxx[t];
            r3[t] = b.obs[g][t] ? r3[t] : pxy[t];
            r4[t] = b.obs[g][t] ? r4[t] : pyy[t];
        }
    }
    b.p2[g] = r2;
    b.p3[g] = r3;
    b.p4[g] = r4;
}

// update NB prepared batches with one particle's pose and store them to its row (FULL batches only: every lane's landmarks
// lie inside the padded row; landmarks beyond L count as "not observed", padding is copied along).  Per particle there is
// the observed point in the world frame, the innovation, the new mean and the likelihood term (ekf_particle); the values
// are those of ekf_update_one + ekf_select.
template <int NB>
__device__ __forceinline__ void ekf_apply(const EkfBatch<NB>& b, const EkfPose& w, int pl, v2f& acc)
{
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        v2f r0 = b.mx[g], r1 = b.my[g];
        if (b.any_obs[g]) {
            const EkfParticle<v2f> u = ekf_particle<v2f>(b.sh[g], b.mx[g], b.my[g], b.zx[g], b.zy[g], w.s, w.c, w.px, w.py);
            v2f ll = u.ll;
            r0 = u.o0;
            r1 = u.o1;
            if (b.any_first[g]) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    r0[t] = b.first[g][t] ? u.wx[t] : r0[t];
                    r1[t] = b.first[g][t] ? u.wy[t] : r1[t];
                    ll[t] = b.first[g][t] ? 0.0f : ll[t];
                }
            }
            if (!b.all_obs[g]) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    r0[t] = b.obs[g][t] ? r0[t] : b.mx[g][t];
                    r1[t] = b.obs[g][t] ? r1[t] : b.my[g][t];
                    ll[t] = b.obs[g][t] ? ll[t] : 0.0f;
                }
            }
            acc = acc + ll;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            row_store(w.rout, b.off[g][t], 0 * pl, r0[t]);
            row_store(w.rout, b.off[g][t], 1 * pl, r1[t]);
            row_store(w.rout, b.off[g][t], 2 * pl, b.p2[g][t]);
            row_store(w.rout, b.off[g][t], 3 * pl, b.p3[g][t]);
            row_store(w.rout, b.off[g][t], 4 * pl, b.p4[g][t]);
        }
    }
}

__device__ __forceinline__ float lane_value(float v, int k)   // lane k's value, wave-uniform (v_readlane_b32)
{
    return __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)__float_as_uint(v), k));
}

// kEkfGroupNb: batches of 128 landmarks a wavefront of the grouped kernels holds in registers per pass; kEkfGroupWpe: waves
// per SIMD the register allocation is held to.  With the pose-independent part of the update hoisted (ekf_prepare) a batch
// costs 13 register pairs: two batches need 97 VGPRs (5 waves at 96 with two dwords of scratch), one batch 69 (7 waves).
// Interleaved A/B on one box (profiles/ab.py, 64k x 500 in the filter): 2 batches at 5 waves — fused front 125.7 us
// (0.1558 ms per frame), update alone 122-134 us; 1 batch at 7 waves — fused front 143.8 us (0.1678 ms), update alone
// 125 us; 1M x 1000: 4.23 against 4.31 ms fused, 4.19 against 4.30 ms alone.  2 batches at 6 waves spill 13 dwords
// (161-178 us), 1 batch at 8 waves 6 dwords (151-167 us).  Before the hoisting (sensor-frame arithmetic, 80 VGPRs, 2 batches
// at 6 waves): fused front 148-153 us, update alone 133-149 us.
// 4 waves (97 VGPRs, nothing spilled) against 5 on another, slower box: fused front 142.7 against 147.3 us, update alone
// 145.0 against 146.3 us; equal at 2000 landmarks and with 32 of 500 observed.
constexpr int kEkfGroupWpe = 4, kEkfGroupNb = 2;
// the same two for the kernels of the split layout (a batch costs fewer registers there: no covariance planes to carry)
constexpr int kEkfSplitWpe = 5;   // 64k x 500, fused front: 4 waves 97.7 us, 5 waves 94.8 us, 6 waves 99.4 us, 8 waves (spills) 149 us
constexpr int kEkfSplitNb = 2;
// `bid`: the workgroup's index after the XCD-contiguous renumbering; s_acc: per particle of the group the 128 accumulators of
// the specification.  OWN_MOTION (the fused front kernel of a frame, below): the poses are not read from a.x / a.y / a.th but
// worked out here — pose = motion_sample(source pose of the ancestor), the very computation the scoring workgroups of the
// same launch make for the same particle (Philox is counter-based: the same bits) — so that the update waits for nobody.
template <int NB, int G, bool OWN_MOTION>
__device__ __forceinline__ void ekf_group_body(const EkfArgs& a, int bid, float (*s_acc)[G][128], const MotionIO& mio,
                                               const MotionParams& mpar)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g0 = (bid * kEkfWaves + wave) * G;
    if (g0 >= a.n) return;
    const int nslots = a.n - g0 < G ? a.n - g0 : G;
    // lane k prepares particle g0 + k: its source row and the trig of its heading; read back with v_readlane below
    const int mine = g0 + ((int)lane < nslots ? (int)lane : 0);
    const int src_l = a.anc ? a.anc[mine] : mine;
    float st_l, ct_l, px_l, py_l;
    if constexpr (OWN_MOTION) {
        float th_l;
        motion_sample_one(mpar, (uint64_t)mine, mio.sx[src_l], mio.sy[src_l], mio.sth[src_l], px_l, py_l, th_l);
        det_sincosf(th_l, st_l, ct_l);
    } else {
        det_sincosf(a.th[mine], st_l, ct_l);
        px_l = a.x[mine];
        py_l = a.y[mine];
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        s_acc[wave][k][lane] = 0.0f;
        s_acc[wave][k][lane + 64] = 0.0f;
    }
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const gchar* ozx = uniform_gptr(a.obs_zx);
    const gchar* ozy = uniform_gptr(a.obs_zy);
    const unsigned L = (unsigned)a.nlandmarks, room = (unsigned)a.plane_stride;
    const v2f q2 = bc2(a.meas_var);
    const float nan = __uint_as_float(0x7fc00000u);

    auto pose_of = [&](int k) {
        EkfPose w;
        const int i = g0 + k;
        w.rout = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_out + (int64_t)i * a.row_stride), 0, row_bytes, 0x00020000);
        w.s = bc2(lane_value(st_l, k));
        w.c = bc2(lane_value(ct_l, k));
        w.px = bc2(lane_value(px_l, k));
        w.py = bc2(lane_value(py_l, k));
        return w;
    };

    unsigned lb = 0;
    for (; lb < L && lb + 128u * NB <= room; lb += 128u * NB) {
        EkfBatch<NB> b;
        // the observations of these landmarks: the same for every particle of the group
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned l = lb + (unsigned)g * 128u + 64u * t + lane;
                const bool in = l < L;
                b.off[g][t] = l * 4u;
                const unsigned zo = (in ? l : 0u) * 4u;   // clamped index + select instead of a predicated load
                const float vx = *(const gfloat*)(ozx + zo), vy = *(const gfloat*)(ozy + zo);
                b.zx[g][t] = in ? vx : nan;
                b.zy[g][t] = in ? vy : nan;
                b.obs[g][t] = b.zx[g][t] == b.zx[g][t] && b.zy[g][t] == b.zy[g][t];
            }
#pragma unroll
        for (int g = 0; g < NB; ++g) {
            b.any_obs[g] = __ballot(b.obs[g][0] || b.obs[g][1]) != 0;
            b.all_obs[g] = __ballot(!(b.obs[g][0] && b.obs[g][1])) == 0;
        }
        int prev = -1;
        for (int k = 0; k < nslots; ++k) {
            const int src = __builtin_amdgcn_readlane(src_l, k);
            if (src != prev) {   // a new ancestor: its batch into registers (wave-uniform branch)
                const __amdgpu_buffer_rsrc_t rin =
                    __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_in + (int64_t)src * a.row_stride), 0, row_bytes, 0x00020000);
                v2f pr[NB][3];
#pragma unroll
                for (int g = 0; g < NB; ++g)
#pragma unroll
                    for (int t = 0; t < 2; ++t) {
                        b.mx[g][t] = row_load(rin, b.off[g][t], 0 * pl);
                        b.my[g][t] = row_load(rin, b.off[g][t], 1 * pl);
#pragma unroll
                        for (int p = 0; p < 3; ++p) pr[g][p][t] = row_load(rin, b.off[g][t], (2 + p) * pl);
                    }
#pragma unroll
                for (int g = 0; g < NB; ++g) ekf_prepare<NB>(b, g, pr[g][0], pr[g][1], pr[g][2], q2);
                prev = src;
            }
            const EkfPose w = pose_of(k);
            v2f acc = (v2f){s_acc[wave][k][lane], s_acc[wave][k][lane + 64]};
            ekf_apply<NB>(b, w, pl, acc);
            s_acc[wave][k][lane] = acc[0];
            s_acc[wave][k][lane + 64] = acc[1];
        }
    }
    // what is left of the rows (a tail shorter than NB batches) and the reduction: particle by particle, general form
    for (int k = 0; k < nslots; ++k) {
        const int i = g0 + k;
        const int src = __builtin_amdgcn_readlane(src_l, k);
        EkfLane w;
        w.rin = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_in + (int64_t)src * a.row_stride), 0, row_bytes, 0x00020000);
        const EkfPose pw = pose_of(k);
        w.rout = pw.rout;
        w.pl = pl;
        w.ozx = ozx;
        w.ozy = ozy;
        w.L = L;
        w.s = pw.s; w.c = pw.c; w.px = pw.px; w.py = pw.py; w.q = q2;
        v2f acc = (v2f){s_acc[wave][k][lane], s_acc[wave][k][lane + 64]};
        unsigned lt = lb;
        for (; lt < L && lt + 128u <= room; lt += 128u) ekf_batches<1, true, true>(w, lt, lane, acc);
        for (; lt < L; lt += 128u) ekf_batches<1, false, true>(w, lt, lane, acc);
        const float total = wave_xor_tree_sum(acc[0] + acc[1]);
        if (lane == 0) {
            a.loglik[i] = total;
            if (a.loglik_user) a.loglik_user[i] = total;
        }
    }
}

template <int NB, int G>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(kEkfGroupWpe, kEkfGroupWpe)))
void ekf_update_group_kernel(EkfArgs a)
{
    __shared__ float s_acc[kEkfWaves][G][128];
    int bid = blockIdx.x;
    if (a.xcd_chunk > 0) bid = (bid & 7) * a.xcd_chunk + (bid >> 3);   // each XCD a contiguous eighth (see ekf_update_kernel)
    ekf_group_body<NB, G, false>(a, bid, s_acc, MotionIO{}, MotionParams{});
}

// ---- the same grouped update on the SPLIT layout (EkfArgs::cov != nullptr): a particle's row holds its landmark MEANS only,
// the covariance planes exist once per covariance class (kernels.h; the classes' own update: split_kernels.hip).  Per particle
// and landmark the update then reads 8 bytes (the ancestor's means, kept in registers for the offspring in the group) and
// writes 8, instead of 20 and 20; the class's covariance row — the same few KB for every wavefront once the population
// descends from few classes — comes out of L2.  Arithmetic, operation order and log-likelihood summation are those of
// ekf_group_body (ekf_shared + ekf_particle): the same bits.  Rows are walked in whole passes of NB batches up to L; lanes
// whose landmarks lie beyond the row's planes get the buffer offset 0xffffffff, which the hardware's range check turns into
// "load 0, drop the store" (score_body.h uses the same device), so no pass needs a predicated form.
template <int NB>
struct SplitBatch {
    v2f mx[NB], my[NB];        // prior means of the current source row
    EkfShared<v2f> sh[NB];     // the pose-independent part of the update, from the current class's covariance row (o2 .. o4 unused)
    v2f zx[NB], zy[NB];
    // the two special cases of a landmark, as lane masks: `keep` = no observation (the prior mean stays, no likelihood term),
    // `first` = observed for the first time (the observed point becomes the mean, no likelihood term); wave-uniform: whether a
    // batch holds any observation at all, and whether it holds a special lane
    bool keep[NB][2], first[NB][2];
    bool any_obs[NB], any_keep[NB], special[NB];
    unsigned off[NB][2];
};

// One batch of one particle.  SPECIAL = false: every lane holds an observed landmark seen before — the plain update, no
// select anywhere.  In a running filter that is nearly every batch, and left to itself the compiler turns the two wave-uniform
// tests around the special cases into 26 v_cndmask per batch (as many instructions as the update's arithmetic: counted in
// the ISA of round 3's kernel): hence two copies of the batch, chosen by a REAL branch (the asm statement keeps the copies
// from being merged back into one).
template <int NB, bool SPECIAL>
__device__ __forceinline__ void split_apply_one(const SplitBatch<NB>& b, int g, const EkfPose& w, int pl, v2f& term)
{
    v2f zx = b.zx[g];
    if constexpr (SPECIAL) asm volatile("" : "+v"(zx));
    const EkfParticle<v2f> u = ekf_particle<v2f>(b.sh[g], b.mx[g], b.my[g], zx, b.zy[g], w.s, w.c, w.px, w.py);
    v2f r0 = u.o0, r1 = u.o1, ll = u.ll;
    if constexpr (!SPECIAL) {
        // The two landmarks of a lane are stored one by one, and left to itself the compiler pushes the two extracts up through
        // the whole expression and then packs each landmark's w00 * dx + w01 * dy as ONE product pair + a horizontal add — with
        // two register moves per pair to line the operands up: 20 instructions for the four new means where 8 packed ones do
        // (counted in the ISA, profiles/r04_split_tuning.md section 10).  The packed values are made opaque before the extracts.
        // Re-checked since the new mean is w - q S^-1 d (no gain W): ekf_split_kernel compiles to the same code without these
        // two statements, the split frame-front kernels do not, so they stay.
        asm("" : "+v"(r0));
        asm("" : "+v"(r1));
    }
    if constexpr (SPECIAL) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {   // obs ? (first ? the observed point : the update) : the prior
            r0[t] = b.keep[g][t] ? b.mx[g][t] : (b.first[g][t] ? u.wx[t] : r0[t]);
            r1[t] = b.keep[g][t] ? b.my[g][t] : (b.first[g][t] ? u.wy[t] : r1[t]);
            ll[t] = (b.keep[g][t] || b.first[g][t]) ? 0.0f : ll[t];
        }
    }
    term = ll;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        row_store(w.rout, b.off[g][t], 0, r0[t]);
        row_store(w.rout, b.off[g][t], pl, r1[t]);
    }
}

// one particle, the NB batches of a pass: term[g] = the batch's log-likelihood terms (+0 where there is none)
template <int NB>
__device__ __forceinline__ void split_apply_terms(const SplitBatch<NB>& b, const EkfPose& w, int pl, v2f (&term)[NB])
{
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        term[g] = bc2(0.0f);
        if (!b.any_obs[g]) {   // nothing observed among these 128 landmarks: the means are copied
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                row_store(w.rout, b.off[g][t], 0, b.mx[g][t]);
                row_store(w.rout, b.off[g][t], pl, b.my[g][t]);
            }
        } else if (b.special[g]) {
            split_apply_one<NB, true>(b, g, w, pl, term[g]);
        } else {
            split_apply_one<NB, false>(b, g, w, pl, term[g]);
        }
    }
}

template <int NB>
__device__ __forceinline__ void split_apply(const SplitBatch<NB>& b, const EkfPose& w, int pl, v2f& acc)
{
    v2f term[NB];
    split_apply_terms<NB>(b, w, pl, term);
#pragma unroll
    for (int g = 0; g < NB; ++g) acc = acc + term[g];   // (a batch without observations adds +0: the bits stay)
}

template <int NB, int G, bool OWN_MOTION>
__device__ __forceinline__ void ekf_split_body(const EkfArgs& a, int bid, float (*s_acc)[G][128], const MotionIO& mio,
                                               const MotionParams& mpar)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int g0 = (bid * kEkfWaves + wave) * G;
    if (g0 >= a.n) return;
    const int nslots = a.n - g0 < G ? a.n - g0 : G;
    // lane k prepares particle g0 + k: source row, class, pose; read back with v_readlane below
    const int mine = g0 + ((int)lane < nslots ? (int)lane : 0);
    const int src_l = a.anc ? a.anc[mine] : mine;
    if (a.group_filter) {   // sharded: this launch takes the groups fed from local rows only (1) or the others (2)
        const bool remote = __ballot(src_l >= a.n) != 0;
        if (remote != (a.group_filter == 2)) return;
    }
    const int cls_l = a.cls_in[src_l];
    float st_l, ct_l, px_l, py_l;
    if constexpr (OWN_MOTION) {
        // the ancestor's POSE comes through the scorer's index (a sharded session reads it out of the all-gathered poses of
        // every rank; on one GPU the two indices are the same array)
        const int psrc = mio.anc ? mio.anc[mine] : mine;
        float th_l;
        motion_sample_one(mpar, (uint64_t)mine, mio.sx[psrc], mio.sy[psrc], mio.sth[psrc], px_l, py_l, th_l);
        det_sincosf(th_l, st_l, ct_l);
    } else {
        det_sincosf(a.th[mine], st_l, ct_l);
        px_l = a.x[mine];
        py_l = a.y[mine];
    }
    if ((int)lane < nslots) {   // the class follows the particle and is still in use
        a.cls_out[mine] = cls_l;
        a.cstamp[cls_l] = a.stamp_now;
    }
#pragma unroll
    for (int k = 0; k < G; ++k) {
        s_acc[wave][k][lane] = 0.0f;
        s_acc[wave][k][lane + 64] = 0.0f;
    }
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const int mean_bytes = 2 * pl, cov_bytes = 3 * pl;
    const gchar* ozx = uniform_gptr(a.obs_zx);
    const gchar* ozy = uniform_gptr(a.obs_zy);
    const unsigned L = (unsigned)a.nlandmarks, room = (unsigned)a.plane_stride;
    const v2f q2 = bc2(a.meas_var);
    const float nan = __uint_as_float(0x7fc00000u);

    auto pose_of = [&](int k) {
        EkfPose w;
        const int i = g0 + k;
        w.rout = __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_out + (int64_t)i * a.row_stride), 0, mean_bytes, 0x00020000);
        w.s = bc2(lane_value(st_l, k));
        w.c = bc2(lane_value(ct_l, k));
        w.px = bc2(lane_value(px_l, k));
        w.py = bc2(lane_value(py_l, k));
        return w;
    };

    // What a pass needs from memory before it can start: the observations of its landmarks, the means of the group's first
    // ancestor and the covariance row of its class, all issued together.  (Issuing the loads of pass p + 1 before pass p is
    // worked on was built and measured: 99.2 against 97.7 us for the fused front at 64k x 500, at 44 more VGPRs — the kernel is
    // bound by its vector instructions, 61 us of them at 64k x 500, and by the drain of its row stores, which a load phase
    // behind them has to wait for on this hardware; removed.)
    struct Raw {
        v2f zx[NB], zy[NB], mx[NB], my[NB], pr[NB][5];
        unsigned off[NB][2];
        bool in[NB][2];
    };
    const int src0 = __builtin_amdgcn_readlane(src_l, 0), cls0 = __builtin_amdgcn_readlane(cls_l, 0);
    auto load_means = [&](int src, const unsigned (&off)[NB][2], v2f (&mx)[NB], v2f (&my)[NB]) {
        const __amdgpu_buffer_rsrc_t rin =
            __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_in + (int64_t)src * a.row_stride), 0, mean_bytes, 0x00020000);
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                mx[g][t] = row_load(rin, off[g][t], 0);
                my[g][t] = row_load(rin, off[g][t], pl);
            }
    };
    auto load_cov = [&](int cls, const unsigned (&off)[NB][2], v2f (&pr)[NB][5]) {
        const __amdgpu_buffer_rsrc_t rc =
            __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.cov + (int64_t)cls * a.cov_stride), 0, cov_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rx =
            __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.covx + (int64_t)cls * a.covx_stride), 0, 2 * pl, 0x00020000);
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
#pragma unroll
                for (int p = 0; p < 3; ++p) pr[g][p][t] = row_load(rc, off[g][t], p * pl);
                pr[g][3][t] = row_load(rx, off[g][t], 0);
                pr[g][4][t] = row_load(rx, off[g][t], pl);
            }
    };
    auto issue = [&](unsigned lb, Raw& r) {
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned l = lb + (unsigned)g * 128u + 64u * t + lane;
                r.in[g][t] = l < L;
                r.off[g][t] = l < room ? l * 4u : 0xffffffffu;   // beyond the planes: loads give 0, stores are dropped
                const unsigned zo = (r.in[g][t] ? l : 0u) * 4u;
                r.zx[g][t] = *(const gfloat*)(ozx + zo);
                r.zy[g][t] = *(const gfloat*)(ozy + zo);
            }
        load_means(src0, r.off, r.mx, r.my);
        load_cov(cls0, r.off, r.pr);
    };
    // everything about the update that depends on the class's covariances alone
    auto prepare = [&](SplitBatch<NB>& b, const v2f (&pr)[NB][5]) {
#pragma unroll
        for (int g = 0; g < NB; ++g) {
            b.first[g][0] = pr[g][0][0] < 0.0f;
            b.first[g][1] = pr[g][0][1] < 0.0f;
            b.special[g] = b.any_keep[g] || __ballot(b.first[g][0] || b.first[g][1]) != 0;
            if (b.any_obs[g]) b.sh[g] = ekf_shared_from<v2f, false>(pr[g][0], pr[g][1], pr[g][2], q2, pr[g][3], pr[g][4]);
        }
    };

    constexpr unsigned kStep = 128u * NB;
    for (unsigned lb = 0; lb < L; lb += kStep) {
        Raw cur;
        issue(lb, cur);
        SplitBatch<NB> b;
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                b.off[g][t] = cur.off[g][t];
                b.zx[g][t] = cur.in[g][t] ? cur.zx[g][t] : nan;
                b.zy[g][t] = cur.in[g][t] ? cur.zy[g][t] : nan;
                b.keep[g][t] = !(b.zx[g][t] == b.zx[g][t] && b.zy[g][t] == b.zy[g][t]);
                b.mx[g][t] = cur.mx[g][t];
                b.my[g][t] = cur.my[g][t];
            }
#pragma unroll
        for (int g = 0; g < NB; ++g) {
            b.any_obs[g] = __ballot(!(b.keep[g][0] && b.keep[g][1])) != 0;
            b.any_keep[g] = __ballot(b.keep[g][0] || b.keep[g][1]) != 0;
        }
        prepare(b, cur.pr);
        int prev = src0, prev_cls = cls0;
        for (int k = 0; k < nslots; ++k) {
            const int src = __builtin_amdgcn_readlane(src_l, k);
            const int cls = __builtin_amdgcn_readlane(cls_l, k);
            if (src != prev) {   // another ancestor: its means into registers (wave-uniform branch)
                load_means(src, b.off, b.mx, b.my);
                prev = src;
            }
            if (cls != prev_cls) {   // another class: its covariances with their determinant terms
                v2f pr[NB][5];
                load_cov(cls, b.off, pr);
                prepare(b, pr);
                prev_cls = cls;
            }
            const EkfPose w = pose_of(k);
            v2f acc = (v2f){s_acc[wave][k][lane], s_acc[wave][k][lane + 64]};
            split_apply<NB>(b, w, pl, acc);
            s_acc[wave][k][lane] = acc[0];
            s_acc[wave][k][lane + 64] = acc[1];
        }
    }
    // the G sums side by side (wave_xor_tree_sum for every particle, the steps interleaved: one after the other they were 6 G
    // dependent cross-lane round trips at the end of every wavefront's life); slots beyond nslots hold zeros
    float tot[G];
#pragma unroll
    for (int k = 0; k < G; ++k) tot[k] = s_acc[wave][k][lane] + s_acc[wave][k][lane + 64];
#pragma unroll
    for (int s = 1; s < 64; s <<= 1)
#pragma unroll
        for (int k = 0; k < G; ++k) tot[k] = tot[k] + __shfl_xor(tot[k], s, 64);
    float total = 0.0f;   // lane k: the sum of particle g0 + k (every lane holds all of them)
#pragma unroll
    for (int k = 0; k < G; ++k) total = (int)lane == k ? tot[k] : total;
    if ((int)lane < nslots) {
        a.loglik[g0 + (int)lane] = total;
        if (a.loglik_user) a.loglik_user[g0 + (int)lane] = total;
    }
}

// (A second form of this update — ONE PASS PER WAVEFRONT: the four wavefronts of a workgroup take the passes of a row side by
// side and share the group's particles, so that no wavefront loads after it has stored; the batches' log-likelihood terms parked
// in LDS and added up in landmark order behind a workgroup barrier, the group's motion samples worked out by one wavefront —
// was built, bit-exact on the whole split suite, and measured slower: fused front 95.5 against 88.6 us at 64k x 500, 2.21
// against 1.80 ms at 1M x 1000 (twice / four times the wavefronts, three barriers per workgroup, 32 KB of LDS that cap the
// occupancy at 4).  Removed; profiles/r04_split_tuning.md.)

template <int NB, int G>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(kEkfSplitWpe, kEkfSplitWpe)))
void ekf_split_kernel(EkfArgs a)
{
    __shared__ float s_acc[kEkfWaves][G][128];
    int bid = blockIdx.x;
    if (a.xcd_chunk > 0) bid = (bid & 7) * a.xcd_chunk + (bid >> 3);
    ekf_split_body<NB, G, false>(a, bid, s_acc, MotionIO{}, MotionParams{});
}

// ---- the FRONT of a single-GPU frame in one launch: motion sample + scan-match score (score_body.h) and the grouped
// out-of-place landmark update side by side.  The two are bound by different units — the scorer by the texture addresser
// (gathers out of L2), the update by HBM writes — and neither needs the other's output: both start from the resample
// indices and the previous poses (the update works out its particles' motion samples itself).  As two launches they run one
// after the other (a second stream with an event fork and join costs more than it wins: DESIGN.md section 11.5); here the
// workgroups of both kinds are dealt out interleaved — of every `score_octets + ekf_octets` consecutive octets of workgroups
// (an octet = one workgroup per XCD) the scoring ones are spread evenly — so the gathers run in the shadow of the row
// stores.  Same bits as the two launches (same device functions).
struct FrontArgs {
    ScoreGrid g;
    const float *bx, *by;
    int nbeams;
    float* score;
    int32_t* count;
    MotionIO mio;
    MotionParams mpar;
    EkfArgs a;
    int score_blocks;    // 256-thread slices of poses to score
    int score_octets;    // ceil(score_blocks / 8)
    int ekf_octets;      // update workgroups per XCD (the xcd_chunk of ekf_update_group_kernel)
    int score_span;      // the scoring octets lie among the first score_span octets of the grid
};

template <int NB, int G, int LPP, int DEPTH, bool SPLIT = false, bool PACKED = false>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(SPLIT ? kEkfSplitWpe : kEkfGroupWpe, SPLIT ? kEkfSplitWpe : kEkfGroupWpe)))
void frame_front_kernel(FrontArgs f)
{
    static_assert(kScoreBlock == kEkfWaves * 64, "both kinds of workgroup have 256 threads");
    extern __shared__ float4 s_pair[];
    __shared__ float s_acc[kEkfWaves][G][128];
    const int o = (int)blockIdx.x >> 3, xcd = (int)blockIdx.x & 7;
    // the scoring octets are spread evenly over the first `span` octets of the grid: the whole grid (against the first part of it
    // only — 64k x 500, 4 / 2 particles per updating wavefront: 100 % 130.7 / 158.5 us, 75 % 134.0 / 156.3, 50 % 155.1 / 154.8,
    // 25 % 141.2 / 157.9)
    const int64_t span = f.score_span;
    const int before = o < span ? (int)((int64_t)o * f.score_octets / span) : f.score_octets;             // scoring octets among 0 .. o - 1
    const int upto = o + 1 < span ? (int)((int64_t)(o + 1) * f.score_octets / span) : f.score_octets;    // ... among 0 .. o
    if (upto > before) {   // a scoring octet (wave-uniform, workgroup-uniform)
        const int sb = before * 8 + xcd;
        if (sb >= f.score_blocks) return;
        score_poses_body<false, LPP, DEPTH, true, PACKED>(f.g, f.bx, f.by, f.nbeams, f.mio.x, f.mio.y, f.mio.th, nullptr, f.a.n,
                                                          f.score, f.count, f.mio, f.mpar, sb, s_pair);
    } else if constexpr (SPLIT) {
        ekf_split_body<NB, G, true>(f.a, xcd * f.ekf_octets + (o - before), s_acc, f.mio, f.mpar);
    } else {
        ekf_group_body<NB, G, true>(f.a, xcd * f.ekf_octets + (o - before), s_acc, f.mio, f.mpar);
    }
}

// ---- sparse in-place form: frames that keep their population update only the OBSERVED landmarks, in place.
// Walking the rows in batches of 128 (ekf_batches, in place) runs the whole update arithmetic at full wavefront cost for
// the handful of lanes of a batch that hold an observation and touches every line a batch's observed landmarks lie in
// once per batch.  Here the observations are first compacted into a list sorted by landmark (once per observation
// table, build_obs_list_kernel); a wavefront then owns one particle and a LANE owns an observation (two per lane, as
// float2): gather the five values at that landmark, update, scatter them back — the same arithmetic in the same order.
// The log-likelihood keeps the summation order of the specification (landmark l adds to accumulator l mod 128 in order
// of l): the accumulators live in LDS, and observations that fall into the same accumulator carry a round number
// (how many earlier observations share it) and are added round by round.
struct ObsList {
    const int32_t* id;      // [nobs] landmark of observation k, ascending
    const float *zx, *zy;   // [nobs]
    const int32_t* round;   // [nobs] number of earlier observations with the same id mod 128
    const int32_t* count;   // [2] device: nobs, highest round
};

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

__global__ __launch_bounds__(kEkfWaves * 64) void ekf_sparse_kernel(EkfArgs a, ObsList ol)
{
    __shared__ float s_acc[kEkfWaves][128];
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int bid = blockIdx.x;
    if (a.xcd_chunk > 0) bid = (bid & 7) * a.xcd_chunk + (bid >> 3);
    const int i = bid * kEkfWaves + wave;
    if (i >= a.n) return;
    float st_, ct_;
    det_sincosf(a.th[i], st_, ct_);
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const __amdgpu_buffer_rsrc_t row =   // in place: the particle's own row, read and written
        __builtin_amdgcn_make_buffer_rsrc((void*)uniform_gptr(a.map_out + (int64_t)i * a.row_stride), 0, row_bytes, 0x00020000);
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
    if (lane == 0) {
        a.loglik[i] = total;
        if (a.loglik_user) a.loglik_user[i] = total;
    }
}

// ---- measurement support (slam_profile_copy_ceiling): the access shape of ekf_update_kernel without its arithmetic
__global__ __launch_bounds__(kEkfWaves * 64) void copy_rows_kernel(const float* __restrict__ in, float* __restrict__ out, int n,
                                                                   int plane_stride, int xcd_chunk)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = threadIdx.x >> 6;
    int bid = blockIdx.x;
    if (xcd_chunk > 0) bid = (bid & 7) * xcd_chunk + (bid >> 3);
    const int i = bid * kEkfWaves + wave;
    if (i >= n) return;
    const float* rin = in + (size_t)i * 5 * plane_stride;
    float* rout = out + (size_t)i * 5 * plane_stride;
    for (int lb = 0; lb < plane_stride; lb += 256) {   // two batches of 128 landmarks: every load before the first store
        const int nb = plane_stride - lb >= 256 ? 2 : 1;
        float m[2][2][5];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int p = 0; p < 5; ++p)
                    if (g < nb) m[g][t][p] = rin[p * plane_stride + lb + g * 128 + t * 64 + lane];
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int p = 0; p < 5; ++p)
                    if (g < nb) __builtin_nontemporal_store(m[g][t][p], &rout[p * plane_stride + lb + g * 128 + t * 64 + lane]);
    }
}

// every float whose exponent lies in the fast reciprocal's range (both signs): ekf_rcp_core against the compiler's IEEE
// division, the scalar form and the packed one; out[0] += mismatches, out[1] += values checked
__global__ __launch_bounds__(256) void selftest_reciprocal_kernel(unsigned long long* __restrict__ out)
{
    unsigned long long bad = 0, seen = 0;
    for (uint64_t b = (uint64_t)blockIdx.x * 256 + threadIdx.x; b < (1ull << 32); b += (uint64_t)gridDim.x * 256) {
        const float d = __uint_as_float((uint32_t)b);
        if (!ekf_rcp_in_range(d)) continue;
        const float exact = 1.0f / d;
        const float fast = ekf_rcp_core(d);
        const v2f two = ekf_rcp((v2f){d, -d});   // (every lane here is in range: the packed fast path)
        bad += (__float_as_uint(exact) != __float_as_uint(fast)) || (__float_as_uint(two[0]) != __float_as_uint(exact)) ||
               (__float_as_uint(two[1]) != (__float_as_uint(exact) ^ 0x80000000u));
        ++seen;
    }
    if (bad) atomicAdd(&out[0], bad);
    atomicAdd(&out[1], seen);
}
}  // namespace

hipError_t launch_motion_sample(hipStream_t stream, const float* sx, const float* sy, const float* sth,
                                const int32_t* anc, float* x, float* y, float* th, int n, int64_t first_id,
                                const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame)
{
    if (n <= 0) return hipSuccess;
    const MotionParams mp = make_motion_params(first_id, dp, sigma, seed, frame);
    motion_sample_kernel<<<blocks_for(n), kBlock, 0, stream>>>(sx, sy, sth, anc, x, y, th, n, mp);
    return hipGetLastError();
}

// The grid of a launch whose workgroups own `per_block` particles each, XCD-contiguous numbering (ekf_update_kernel) from 64
// workgroups on: the grid is padded to a multiple of 8 (surplus workgroups exit at once) and xcd_chunk = workgroups per XCD;
// smaller grids stay as they are, xcd_chunk = 0.
static int xcd_grid(int n, int per_block, int& xcd_chunk)
{
    const int blocks = (n + per_block - 1) / per_block;
    xcd_chunk = blocks >= 64 ? (blocks + 7) / 8 : 0;
    return xcd_chunk ? 8 * xcd_chunk : blocks;
}

hipError_t launch_ekf_update(hipStream_t stream, const EkfArgs& a_in, const EventPair* ev, int group_size)
{
    if (a_in.n <= 0) return hipSuccess;
    EkfArgs a = a_in;
    if (a.cov) {   // split layout: always the grouped form (2 particles per wavefront unless the caller asks for 4 or 8)
        const int G = group_size == 4 || group_size == 8 ? group_size : 2;
        const int gblocks = xcd_grid(a.n, kEkfWaves * G, a.xcd_chunk);
        if (ev) (void)hipEventRecord(ev->start, stream);
        if (G == 8) ekf_split_kernel<kEkfSplitNb, 8><<<gblocks, kEkfWaves * 64, 0, stream>>>(a);
        else if (G == 4) ekf_split_kernel<kEkfSplitNb, 4><<<gblocks, kEkfWaves * 64, 0, stream>>>(a);
        else ekf_split_kernel<kEkfSplitNb, 2><<<gblocks, kEkfWaves * 64, 0, stream>>>(a);
        if (ev) (void)hipEventRecord(ev->stop, stream);
        return hipGetLastError();
    }
    const bool copy = a.map_in != a.map_out;   // in place: rows without an observation stay as they are
    // out of place, more than one batch per row: optionally the grouped form (group_size neighbouring particles per
    // wavefront, shared source rows stay in registers); the caller knows roughly how many distinct ancestors the last
    // resample left (slam_ekf_form_set forces one form).
    if (copy && a.nlandmarks > 128 && group_size > 0) {
        // group size: measured on MI355X (64k x 500 | 1M x 1000 | 64k x 500 with 50 % distinct ancestors | 512k x 5000; one
        // wavefront per particle: 156 us | 4.28 ms | 177 us | 10.09 ms): 2 particles 148 | 4.09 | 169 | 9.79; 3: 135;
        // 4: 139 | 3.86 | 180 | 9.82; 6: 141; 8: 150 | 3.84 | 199 | 9.92.  Hence 4 when neighbours share ancestors, 2 when
        // they rarely do.  Batches in flight per pass (the first template argument),
        // group of 4, 64k x 500 | 1M x 1000 | 512k x 5000: 1: 150 us | 3.97 ms; 2: 140-145 | 3.90-3.92 | 9.79; 3: 144 | 4.02;
        // 4: 137-139 | 3.86 | 9.86 — within the run-to-run spread: 2 kept (82 VGPRs, 5 waves per SIMD; 4 needs 114).
        // The engine asks for 2 or 4 on rows (slam_engine::ekf_group_size); any other size gets the 4-particle kernel and its grid.
        const int G = group_size == 2 ? 2 : 4;
        const int gblocks = xcd_grid(a.n, kEkfWaves * G, a.xcd_chunk);
        if (ev) (void)hipEventRecord(ev->start, stream);
        if (G == 2) ekf_update_group_kernel<kEkfGroupNb, 2><<<gblocks, kEkfWaves * 64, 0, stream>>>(a);
        else ekf_update_group_kernel<kEkfGroupNb, 4><<<gblocks, kEkfWaves * 64, 0, stream>>>(a);
        if (ev) (void)hipEventRecord(ev->stop, stream);
        return hipGetLastError();
    }
    // batches of 128 landmarks in flight per wavefront: 2 measured best at 64k x 500 (1: 178 us, 2: 166 us, 4: 180 us)
    const int nb = a.nlandmarks <= 128 ? 1 : 2;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    // in place: 4 batches (512 landmarks) per round trip; measured at 64k x 500 with 32 landmarks observed: 1 batch at a
    // time 91 us, because every batch is its own dependent chain obs table -> row -> store
    if (!copy && a.nlandmarks > 128) ekf_update_kernel<4, false><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else if (!copy) ekf_update_kernel<1, false><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else if (nb == 1) ekf_update_kernel<1, true><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    else ekf_update_kernel<2, true><<<blocks, kEkfWaves * 64, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

bool frame_front_fits(int n, int nlandmarks, int group_size)
{
    if (n < kWaveMaxPoses || nlandmarks <= 128 || (group_size != 2 && group_size != 4 && group_size != 8)) return false;
    return (n + kEkfWaves * group_size - 1) / (kEkfWaves * group_size) >= 64;
}

// The front of a single-GPU frame in one launch (frame_front_kernel).  *launched = false when the shapes do not fit it (few
// particles: the one-wavefront-per-pose scorer; short rows; too few update workgroups for the XCD-contiguous numbering): the
// caller then issues the two launches.
hipError_t launch_frame_front(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                              const MotionIO& io, int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed,
                              uint32_t frame, float* score, int32_t* count, const EkfArgs& a_in, int group_size,
                              const EventPair* ev, bool* launched, int* lanes_per_pose)
{
    *launched = false;
    const int n = a_in.n;
    if (!a_in.cov && group_size == 8) group_size = 4;   // rows: 2 or 4 particles per updating wavefront
    if (a_in.map_in == a_in.map_out || !frame_front_fits(n, a_in.nlandmarks, group_size)) return hipSuccess;
    const int G = group_size;
    const int gblocks = (n + kEkfWaves * G - 1) / (kEkfWaves * G);
    const bool quad = n < kQuadMaxPoses;
    FrontArgs f;
    f.g = g;
    f.bx = bx;
    f.by = by;
    f.nbeams = nbeams;
    f.score = score;
    f.count = count;
    f.mio = io;
    f.mpar = make_motion_params(first_id, dp, sigma, seed, frame);
    f.a = a_in;
    f.ekf_octets = (gblocks + 7) / 8;
    f.a.xcd_chunk = f.ekf_octets;
    f.score_blocks = (int)(((quad ? 4L : 1L) * n + kScoreBlock - 1) / kScoreBlock);
    f.score_octets = (f.score_blocks + 7) / 8;
    f.score_span = f.score_octets + f.ekf_octets;
    const int grid = 8 * f.score_span;
    const size_t lds = sizeof(float2) * (size_t)(nbeams + (quad ? 4 * kQuadDepth : kLaneDepth)) + (g.packed ? 1024 : 0);
    if (ev) (void)hipEventRecord(ev->start, stream);
    // the instantiation: particles per updating wavefront (8: split only) x scorer's lane mapping x map layout x grid copy read
#define SLAM_FRONT(G_, SP_, PK_)                                                                                                  \
    do {                                                                                                                          \
        constexpr int NB_ = (SP_) ? kEkfSplitNb : kEkfGroupNb;                                                                    \
        if (quad) frame_front_kernel<NB_, G_, 4, kQuadDepth, SP_, PK_><<<grid, kEkfWaves * 64, lds, stream>>>(f);                 \
        else frame_front_kernel<NB_, G_, 1, kLaneDepth, SP_, PK_><<<grid, kEkfWaves * 64, lds, stream>>>(f);                      \
    } while (0)
#define SLAM_FRONT_PK(G_, SP_) do { if (f.g.packed) SLAM_FRONT(G_, SP_, true); else SLAM_FRONT(G_, SP_, false); } while (0)
    if (G == 2) { if (f.a.cov) SLAM_FRONT_PK(2, true); else SLAM_FRONT_PK(2, false); }
    else if (G == 8 && f.a.cov) SLAM_FRONT_PK(8, true);
    else if (f.a.cov) SLAM_FRONT_PK(4, true);
    else SLAM_FRONT_PK(4, false);
#undef SLAM_FRONT_PK
#undef SLAM_FRONT
    if (ev) (void)hipEventRecord(ev->stop, stream);
    *launched = true;
    if (lanes_per_pose) *lanes_per_pose = quad ? 4 : 1;
    return hipGetLastError();
}

hipError_t launch_selftest_reciprocal(hipStream_t stream, unsigned long long* out)
{
    selftest_reciprocal_kernel<<<256 * 16, 256, 0, stream>>>(out);
    return hipGetLastError();
}

hipError_t launch_build_obs_list(hipStream_t stream, const float* tzx, const float* tzy, int L, const ObsListOut& ol, int32_t* h_count)
{
    build_obs_list_kernel<<<1, 1024, 0, stream>>>(tzx, tzy, L, ol, h_count);
    return hipGetLastError();
}

hipError_t launch_ekf_sparse(hipStream_t stream, const EkfArgs& a_in, const int32_t* id, const float* zx, const float* zy,
                             const int32_t* round, const int32_t* count, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    EkfArgs a = a_in;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    ObsList ol{ id, zx, zy, round, count };
    if (ev) (void)hipEventRecord(ev->start, stream);
    ekf_sparse_kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a, ol);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_copy_rows(hipStream_t stream, const float* in, float* out, int n, int plane_stride)
{
    const int blocks = (n + kEkfWaves - 1) / kEkfWaves, chunk = (blocks + 7) / 8;
    copy_rows_kernel<<<chunk * 8, kEkfWaves * 64, 0, stream>>>(in, out, n, plane_stride, chunk);
    return hipGetLastError();
}

}  // namespace slam
