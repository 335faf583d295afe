// ekf_split_body.h — the grouped landmark update on the split layout (ekf_split_kernel of ekf_kernels.hip, the updating
// workgroups of the split frame_front_kernel in front_kernels.hip).
// ---- the same grouped update on the SPLIT layout (EkfArgs::cov != nullptr): a particle's row holds its landmark MEANS only,
// the covariance planes exist once per covariance class (kernels.h; the classes' own update: split_kernels.hip).  Per particle
// and landmark the update then reads 8 bytes (the ancestor's means, kept in registers for the offspring in the group) and
// writes 8, instead of 20 and 20; the class's covariance row — the same few KB for every wavefront once the population
// descends from few classes — comes out of L2.  Arithmetic, operation order and log-likelihood summation are those of
// ekf_group_body (ekf_shared + ekf_particle): the same bits.  Rows are walked in whole passes of NB batches up to L; lanes
// whose landmarks lie beyond the row's planes get the buffer offset 0xffffffff, which the hardware's range check turns into
// "load 0, drop the store" (score_body.h uses the same device), so no pass needs a predicated form.
#pragma once

#include "ekf_wave.h"

namespace slam {

// waves per SIMD and batches per pass, as kEkfGroupWpe / kEkfGroupNb of ekf_group_body.h:
// the same two for the kernels of the split layout (a batch costs fewer registers there: no covariance planes to carry)
constexpr int kEkfSplitWpe = 5;   // 64k x 500, fused front: 4 waves 97.7 us, 5 waves 94.8 us, 6 waves 99.4 us, 8 waves (spills) 149 us
constexpr int kEkfSplitNb = 2;
// ... of the front launch that writes no mean row (survivor rows; 69 VGPRs, no scratch at 5, 6 and 7): ms per frame, medians of four
// interleaved runs, 64k x 500: 5 waves 0.0809, 6 waves 0.0790, 7 waves 0.0808; 1M x 1000: 5 waves 1.031, 6 waves 1.000, 7 waves 1.007
// (profiles/r06_survivor_ride.md)
constexpr int kEkfSplitWpeNoStore = 6;

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
// MEANS = false (a survivor-rows frame's front launch): no mean is stored, the log-likelihood terms are all that is left — the
// same terms: the new means are dead values then and go, with the pins that would keep them alive.
template <int NB, bool SPECIAL, bool MEANS>
__device__ __forceinline__ void split_apply_one(const SplitBatch<NB>& b, int g, const EkfPose& w, int pl, v2f& term)
{
    v2f zx = b.zx[g];
    if constexpr (SPECIAL) asm volatile("" : "+v"(zx));
    const EkfParticle<v2f> u = ekf_particle<v2f>(b.sh[g], b.mx[g], b.my[g], zx, b.zy[g], w.s, w.c, w.px, w.py);
    v2f r0 = u.o0, r1 = u.o1, ll = u.ll;
    if constexpr (!SPECIAL && MEANS) {
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
            if constexpr (MEANS) r0[t] = b.keep[g][t] ? b.mx[g][t] : (b.first[g][t] ? u.wx[t] : r0[t]);
            if constexpr (MEANS) r1[t] = b.keep[g][t] ? b.my[g][t] : (b.first[g][t] ? u.wy[t] : r1[t]);
            ll[t] = (b.keep[g][t] || b.first[g][t]) ? 0.0f : ll[t];
        }
    }
    term = ll;
    if constexpr (MEANS) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            row_store(w.rout, b.off[g][t], 0, r0[t]);
            row_store(w.rout, b.off[g][t], pl, r1[t]);
        }
    }
}

// one particle, the NB batches of a pass: term[g] = the batch's log-likelihood terms (+0 where there is none)
template <int NB, bool MEANS>
__device__ __forceinline__ void split_apply_terms(const SplitBatch<NB>& b, const EkfPose& w, int pl, v2f (&term)[NB])
{
#pragma unroll
    for (int g = 0; g < NB; ++g) {
        term[g] = bc2(0.0f);
        if (!b.any_obs[g]) {   // nothing observed among these 128 landmarks: the means are copied
            if constexpr (MEANS) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    row_store(w.rout, b.off[g][t], 0, b.mx[g][t]);
                    row_store(w.rout, b.off[g][t], pl, b.my[g][t]);
                }
            }
        } else if (b.special[g]) {
            split_apply_one<NB, true, MEANS>(b, g, w, pl, term[g]);
        } else {
            split_apply_one<NB, false, MEANS>(b, g, w, pl, term[g]);
        }
    }
}

template <int NB, bool MEANS>
__device__ __forceinline__ void split_apply(const SplitBatch<NB>& b, const EkfPose& w, int pl, v2f& acc)
{
    v2f term[NB];
    split_apply_terms<NB, MEANS>(b, w, pl, term);
#pragma unroll
    for (int g = 0; g < NB; ++g) acc = acc + term[g];   // (a batch without observations adds +0: the bits stay)
}

// MEANS / TALLY: the two halves of what the update leaves, for a survivor-rows frame.  Its front launch runs
// MEANS = false — classes, stamps and log-likelihoods, no mean row —, and the launch behind its resample (ekf_materialise_kernel)
// TALLY = false — mean rows and nothing else, for the particles EkfArgs::survivor names.  The same device functions either way.
// OWN_MOTION (the fused front of a frame): the poses are not read but worked out here, as ekf_group_body does — but ONCE per
// workgroup: one wavefront makes the motion samples and the sines and cosines of the workgroup's kEkfWaves * G particles in its
// low lanes and hands them over in LDS (s_motion: one float4 (x, y, sine, cosine) per particle), where every wavefront for
// itself ran Philox, Box-Muller and det_sincosf in 64 lanes to use G of them.  A particle's sample is a function of its index
// and its ancestor's pose alone: the same bits.  The one barrier this costs stands behind everything a wavefront can issue
// without its poses — the gather indices, the classes, the loads of its first pass —, so the round trips of those run while
// the samples are made; every wavefront of a workgroup with a particle reaches it, also one that has no particle of its own
// or whose group this launch leaves out (group_filter).
// OWN_MOTION = kPosesStaged (frame_particle_kernel of front_kernels.hip, whose workgroups score their particles first): the samples
// lie in s_motion already, behind a barrier of the caller's — nothing is made here and nothing waited for.
// ekf_split_group is the update of ONE group: the G particles from `first + slot * G` on, `first` the first particle of the
// workgroup, whose samples s_motion holds from particle `first` on; wavefront `wave` of the workgroup works on it, with
// s_acc[wave].  A wavefront may take several groups one after the other (kPosesStaged, kPosesRead: no barrier inside).
// s_ll (optional, TALLY): the group's log-likelihood totals are left in s_ll[slot * G ...] as well, for a later phase of the workgroup.
enum : int { kPosesRead = 0, kPosesMade = 1, kPosesStaged = 2 };

template <int NB, int G, int OWN_MOTION, bool MEANS = true, bool TALLY = true>
__device__ __forceinline__ void ekf_split_group(const EkfArgs& a, int first, int slot, int wave, float (*s_acc)[G][128],
                                                const MotionIO& mio, const MotionParams& mpar, float4* s_motion = nullptr,
                                                float* s_ll = nullptr)
{
    const unsigned lane = threadIdx.x & 63u;
    const int g0 = first + slot * G;
    if (first >= a.n) return;   // (a surplus workgroup of the padded grid: all its wavefronts leave)
    bool skip = g0 >= a.n;      // wave-uniform: nothing to update here
    if constexpr (OWN_MOTION != kPosesMade)
        if (skip) return;
    const int nslots = skip ? 0 : a.n - g0 < G ? a.n - g0 : G;
    // lane k prepares particle g0 + k: source row, class, pose; read back with v_readlane below
    const int mine = skip ? first : g0 + ((int)lane < nslots ? (int)lane : 0);
    unsigned long long alive = ~0ull;   // (TALLY = false) the group's particles that get a row
    if constexpr (!TALLY) {
        if (a.survivor) alive = __ballot((int)lane < nslots && a.survivor[mine] == a.survivor_stamp);
        if (alive == 0) return;   // nobody here survived the resample
    }
    const int k0 = TALLY ? 0 : __builtin_amdgcn_readfirstlane(__builtin_ctzll(alive));   // the first particle worked on
    const int src_l = a.anc ? a.anc[mine] : mine;
    if (a.group_filter) {   // sharded: this launch takes the groups fed from local rows only (1) or the others (2)
        const bool remote = __ballot(src_l >= a.n) != 0;
        if (remote != (a.group_filter == 2)) {
            if constexpr (OWN_MOTION != kPosesMade) return;
            skip = true;
        }
    }
    const int cls_l = a.cls_in[OWN_MOTION == kPosesMade && skip ? mine : src_l];   // (a group left out may have its source rows elsewhere)
    const int pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    const int mean_bytes = 2 * pl, cov_bytes = 3 * pl;
    const gchar* ozx = uniform_gptr(a.obs_zx);
    const gchar* ozy = uniform_gptr(a.obs_zy);
    const unsigned L = (unsigned)a.nlandmarks, room = (unsigned)a.plane_stride;
    const v2f q2 = bc2(a.meas_var);
    const float nan = __uint_as_float(0x7fc00000u);

    float st_l, ct_l, px_l, py_l;   // lane k: the pose of particle g0 + k (set below)
    auto pose_of = [&](int k) {
        EkfPose w;
        w.rout = row_rsrc(a.map_out, g0 + k, a.row_stride, mean_bytes);
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
    const int src0 = __builtin_amdgcn_readlane(src_l, k0), cls0 = __builtin_amdgcn_readlane(cls_l, k0);
    auto load_means = [&](int src, const unsigned (&off)[NB][2], v2f (&mx)[NB], v2f (&my)[NB]) {
        const __amdgpu_buffer_rsrc_t rin = row_rsrc(a.map_in, src, a.row_stride, mean_bytes);
#pragma unroll
        for (int g = 0; g < NB; ++g)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                mx[g][t] = row_load(rin, off[g][t], 0);
                my[g][t] = row_load(rin, off[g][t], pl);
            }
    };
    auto load_cov = [&](int cls, const unsigned (&off)[NB][2], v2f (&pr)[NB][5]) {
        const __amdgpu_buffer_rsrc_t rc = row_rsrc(a.cov, cls, a.cov_stride, cov_bytes);
        const __amdgpu_buffer_rsrc_t rx = row_rsrc(a.covx, cls, a.covx_stride, 2 * pl);
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
    Raw cur;   // the loads of a pass are issued at the end of the pass before it; those of the first one ahead of the poses
    if constexpr (OWN_MOTION == kPosesMade) {
        if (wave == 0) {   // particle first + lane in lane < kEkfWaves * G: the whole workgroup's samples in one wavefront
            const int i = first + (int)lane;
            if ((int)lane < kEkfWaves * G && i < a.n) {
                // the ancestor's POSE comes through the scorer's index (a sharded session reads it out of the all-gathered poses
                // of every rank; on one GPU the two indices are the same array)
                const int psrc = mio.anc ? mio.anc[i] : i;
                float x, y, th, st, ct;
                motion_sample_one(mpar, (uint64_t)i, mio.sx[psrc], mio.sy[psrc], mio.sth[psrc], x, y, th);
                det_sincosf(th, st, ct);
                s_motion[lane] = make_float4(x, y, st, ct);
            }
        }
        // (behind the samples in wavefront 0: in front of them the 40 registers the loads land in stay reserved through
        // Philox — 73 VGPRs and a stack object instead of 72 and none; its gather index and class are on their way meanwhile)
        if (!skip && L > 0) issue(0, cur);
        __syncthreads();
        if (skip) return;
    } else {
        if (L > 0) issue(0, cur);
    }
    if constexpr (OWN_MOTION != kPosesRead) {
        const float4 m = s_motion[slot * G + ((int)lane < nslots ? (int)lane : 0)];
        px_l = m.x;
        py_l = m.y;
        st_l = m.z;
        ct_l = m.w;
    } else {
        det_sincosf(a.th[mine], st_l, ct_l);
        px_l = a.x[mine];
        py_l = a.y[mine];
    }
    if constexpr (TALLY) {
        if ((int)lane < nslots) {   // the class follows the particle and is still in use
            a.cls_out[mine] = cls_l;
            a.cstamp[cls_l] = a.stamp_now;
        }
#pragma unroll
        for (int k = 0; k < G; ++k) acc_store<G>(s_acc, wave, k, lane, bc2(0.0f));
    }
    for (unsigned lb = 0; lb < L;) {
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
        for (int k = k0; k < nslots; ++k) {
            if constexpr (!TALLY)
                if (!((alive >> k) & 1ull)) continue;
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
            if constexpr (TALLY) {
                v2f acc = acc_load<G>(s_acc, wave, k, lane);
                split_apply<NB, MEANS>(b, w, pl, acc);
                acc_store<G>(s_acc, wave, k, lane, acc);
            } else {
                v2f term[NB];
                split_apply_terms<NB, true>(b, w, pl, term);
            }
        }
        lb += kStep;
        if (lb < L) issue(lb, cur);
    }
    if constexpr (!TALLY) return;
    // the G sums side by side (wave_xor_tree_sum's bits for every particle, on the halving schedule of ekf_wave.h: one after the
    // other the butterflies were 6 G dependent cross-lane round trips at the end of every wavefront's life, interleaved still
    // 6 G exchanges and additions, half of them made twice); slots beyond nslots hold zeros
    float tot[G];
#pragma unroll
    for (int k = 0; k < G; ++k) {
        const v2f acc = acc_load<G>(s_acc, wave, k, lane);
        tot[k] = acc[0] + acc[1];
    }
    const float total = wave_halving_tree_sums<G>(tot, lane);   // lane k < G: the sum of particle g0 + k
    if ((int)lane < nslots) {
        store_loglik(a, g0 + (int)lane, total);
        if (s_ll) s_ll[slot * G + (int)lane] = total;
    }
}

// a workgroup of kEkfWaves wavefronts with one group each: workgroup `bid` takes the particles from bid * kEkfWaves * G on
template <int NB, int G, int OWN_MOTION, bool MEANS = true, bool TALLY = true>
__device__ __forceinline__ void ekf_split_body(const EkfArgs& a, int bid, float (*s_acc)[G][128], const MotionIO& mio,
                                               const MotionParams& mpar, float4* s_motion = nullptr)
{
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    ekf_split_group<NB, G, OWN_MOTION, MEANS, TALLY>(a, bid * kEkfWaves * G, wave, wave, s_acc, mio, mpar, s_motion);
}

// (A second form of this update — ONE PASS PER WAVEFRONT: the four wavefronts of a workgroup take the passes of a row side by
// side and share the group's particles, so that no wavefront loads after it has stored; the batches' log-likelihood terms parked
// in LDS and added up in landmark order behind a workgroup barrier, the group's motion samples worked out by one wavefront —
// was built, bit-exact on the whole split suite, and measured slower: fused front 95.5 against 88.6 us at 64k x 500, 2.21
// against 1.80 ms at 1M x 1000 (twice / four times the wavefronts, three barriers per workgroup, 32 KB of LDS that cap the
// occupancy at 4).  Removed; profiles/r04_split_tuning.md.)

}  // namespace slam
