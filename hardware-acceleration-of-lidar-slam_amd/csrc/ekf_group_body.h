// ekf_group_body.h — the grouped form of the out-of-place landmark update on rows (ekf_update_group_kernel of ekf_kernels.hip,
// the updating workgroups of frame_front_kernel in front_kernels.hip).
// ---- grouped form of the out-of-place update: ONE WAVEFRONT OWNS G NEIGHBOURING PARTICLES (G = 2, 4 or 8).
// After a resample the slots are sorted by ancestor, so neighbouring particles mostly descend from the same one.  The
// row-per-wavefront kernel lets them share the source row through L2; measured (profiles/copy_ceiling.hip) even a pure copy
// pays for that — 155 us at 64k x 512 columns when 16 neighbours share a source, against 109 us when nothing is re-read.
// Here the wavefront walks the landmarks in the OUTER loop and its G particles in the inner one: a batch of the source
// row stays in registers while every particle of the group that descends from it is updated with its own pose and stored
// to its own row — the re-reads never leave the register file, the observation table is read once per group.  Per
// (particle, landmark) the arithmetic, its order and the log-likelihood summation are those of ekf_batches (bit-exact:
// the same tests cover both kernels); the per-particle accumulators live in LDS between batches.
#pragma once

#include "ekf_row_body.h"

namespace slam {

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

// `bid`: the workgroup's index after the XCD-contiguous renumbering; s_acc: per particle of the group the 128 accumulators of
// the specification.  OWN_MOTION (the fused front kernel of a frame, front_kernels.hip): the poses are not read from a.x / a.y / a.th but
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
    for (int k = 0; k < G; ++k) acc_store<G>(s_acc, wave, k, lane, bc2(0.0f));
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    const gchar* ozx = uniform_gptr(a.obs_zx);
    const gchar* ozy = uniform_gptr(a.obs_zy);
    const unsigned L = (unsigned)a.nlandmarks, room = (unsigned)a.plane_stride;
    const v2f q2 = bc2(a.meas_var);
    const float nan = __uint_as_float(0x7fc00000u);

    auto pose_of = [&](int k) {
        EkfPose w;
        w.rout = row_rsrc(a.map_out, g0 + k, a.row_stride, row_bytes);
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
                const __amdgpu_buffer_rsrc_t rin = row_rsrc(a.map_in, src, a.row_stride, row_bytes);
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
            v2f acc = acc_load<G>(s_acc, wave, k, lane);
            ekf_apply<NB>(b, w, pl, acc);
            acc_store<G>(s_acc, wave, k, lane, acc);
        }
    }
    // what is left of the rows (a tail shorter than NB batches) and the reduction: particle by particle, general form
    for (int k = 0; k < nslots; ++k) {
        const int i = g0 + k;
        const int src = __builtin_amdgcn_readlane(src_l, k);
        EkfLane w;
        w.rin = row_rsrc(a.map_in, src, a.row_stride, row_bytes);
        w.p = pose_of(k);
        w.pl = pl;
        w.L = L;
        w.noise.q = q2;
        w.obs.ozx = ozx;
        w.obs.ozy = ozy;
        v2f acc = acc_load<G>(s_acc, wave, k, lane);
        unsigned lt = lb;
        for (; lt < L && lt + 128u <= room; lt += 128u) ekf_batches<1, true, true>(w, lt, lane, acc);
        for (; lt < L; lt += 128u) ekf_batches<1, false, true>(w, lt, lane, acc);
        const float total = wave_xor_tree_sum(acc[0] + acc[1]);
        if (lane == 0) store_loglik(a, i, total);
    }
}

}  // namespace slam
