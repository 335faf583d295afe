// ekf_row_body.h — the landmark update with a row per wavefront (ekf_update_kernel of ekf_kernels.hip; the grouped form's
// row tails, ekf_group_body.h).
// The map is one row per particle (5 planes of plane_stride floats).  ONE WAVEFRONT OWNS ONE PARTICLE and its
// lanes walk the landmarks of the row, two landmarks per lane (l and l + 64 of each batch of 128), so that every
// load and store is a coalesced 256-byte access and the arithmetic runs on float2 (v_pk_mul_f32 / v_pk_add_f32:
// IEEE per component, i.e. the same bits as the scalar form).  The observations of the frame come as a table indexed by
// landmark (zx[l], zy[l], NaN = not observed), read alongside the row.  Why rows: after a resample most
// particles are copies of few ancestors (the bench's filter keeps ~6 % distinct), the offspring of one ancestor
// are neighbouring particles, so the 10 KB source row is fetched from HBM once and re-read from L2 by the other
// offspring — the sweep's HBM traffic is the 20 B/(particle, landmark) it writes plus the distinct rows it reads,
// not 40 B.  Row base addresses are wave-uniform (SGPR).
#pragma once

#include "ekf_wave.h"

namespace slam {

// What goes into the row for the two landmarks of a lane, given the update's result in r0 .. r4 / ll: a first sighting
// (prior P_xx < 0) takes the observed point and P = (fxx, fxy, fyy) — q I, or the particle's R_w when the measurement covariance
// is a full 2x2 (ekf_aniso_lane.h) — and adds no likelihood term; a landmark without an observation keeps
// its prior values.  Both cases are decided for the WAVEFRONT first (a ballot each): in a running filter most batches of
// 128 landmarks hold neither — every landmark seen before, every one observed, or none — and then the selects (and the
// arithmetic of the first sighting) are skipped altogether.  The values are those of
//     ob ? (first ? {f0, f1, fxx, fxy, fyy; 0} : {o0 .. o4; ll}) : {prior; 0}
// in every case.
__device__ __forceinline__ void ekf_select(v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll, v2f mx, v2f my, v2f pxx, v2f pxy,
                                           v2f pyy, v2f zx, v2f zy, v2f s, v2f c, v2f px, v2f py, v2f fxx, v2f fxy, v2f fyy, bool ob0,
                                           bool ob1)
{
    if (__ballot(pxx[0] < 0.0f || pxx[1] < 0.0f) != 0) {
        v2f f0, f1;
        ekf_first_sighting<v2f>(zx, zy, s, c, px, py, f0, f1);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const bool first = pxx[t] < 0.0f;
            r0[t] = first ? f0[t] : r0[t];
            r1[t] = first ? f1[t] : r1[t];
            r2[t] = first ? fxx[t] : r2[t];
            r3[t] = first ? fxy[t] : r3[t];
            r4[t] = first ? fyy[t] : r4[t];
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

// A wavefront's lane type is made of two independent choices, each a policy with the kernel argument it needs beyond EkfArgs
// (Args), an init() for one particle and the one operation ekf_batches asks of it.
//
// NOISE — the measurement noise and the arithmetic per landmark.  This one: meas_var * I (a first sighting stores P = q I);
// EkfNoiseAniso of ekf_aniso_lane.h: the particle's R_w from a 2x2 sensor-frame Q; EkfNoiseDet there: from the Q_k of the detection
// each landmark takes, which the lane fetches (fetch) beside z while the row's loads are issued and keeps in an Aux per batch.
struct EkfNoiseIso {
    struct Args {};   // a.meas_var is all it needs
    struct Aux {};    // what a lane keeps per batch beside z for its two landmarks: nothing (EkfNoiseDet: their detections' Q)
    v2f q;
    __device__ __forceinline__ void init(const EkfArgs& a, const Args&, float s, float c) { q = bc2(a.meas_var); }
    template <class OBS> __device__ __forceinline__ void fetch(const OBS&, unsigned l, bool in, int t, Aux&) const {}
    // what goes into the row for the two landmarks of a lane (ob0 / ob1: they have an observation) and their likelihood terms
    __device__ __forceinline__ void update(const EkfPose& p, v2f mx, v2f my, v2f pxx, v2f pxy, v2f pyy, v2f zx, v2f zy, const Aux&, bool ob0, bool ob1,
                                           v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll) const
    {
        const EkfResult<v2f> u = ekf_update_one<v2f, false>(mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, q);
        r0 = u.o0; r1 = u.o1; r2 = u.o2; r3 = u.o3; r4 = u.o4; ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, q, bc2(0.0f), q, ob0, ob1);
    }
};

// OBS — the observation of landmark l (in: l < L; NaN = none).  This one: the frame's table indexed by landmark, a.obs_zx / a.obs_zy.
struct EkfObsFrame {
    struct Args {};
    const gchar *ozx, *ozy;
    __device__ __forceinline__ void init(const EkfArgs& a, const Args&, int i, unsigned lane)
    {
        ozx = uniform_gptr(a.obs_zx);
        ozy = uniform_gptr(a.obs_zy);
    }
    __device__ __forceinline__ void get(unsigned l, bool in, float& vx, float& vy) const
    {
        const unsigned zo = (in ? l : 0u) * 4u;   // clamped index + select instead of a predicated load
        vx = *(const gfloat*)(ozx + zo);
        vy = *(const gfloat*)(ozy + zo);
    }
};
// ... and det[assoc[i][l]], the particle's own association table (data association: assoc_kernels.hip makes the table): lane k of
// the wavefront holds detection k (NaN from ndet on), the table byte is read alongside the row and the detection comes from a
// lane read — no second trip to memory.
struct EkfObsTable {
    typedef EkfAssocTable Args;
    const gchar* arow;   // the particle's table row (wave-uniform)
    float detx, dety;    // THIS lane's detection
    __device__ __forceinline__ void init(const EkfArgs& a, const Args& tab, int i, unsigned lane)
    {
        const float nan = __uint_as_float(0x7fc00000u);
        arow = uniform_gptr(tab.assoc + (size_t)i * (size_t)tab.assoc_stride);
        detx = (int)lane < tab.ndet ? tab.det_zx[lane] : nan;
        dety = (int)lane < tab.ndet ? tab.det_zy[lane] : nan;
    }
    // the table byte of landmark l (clamped index: the caller discards what lanes beyond L get) ...
    __device__ __forceinline__ unsigned entry(unsigned l, bool in) const { return *(const guchar*)(arow + (in ? l : 0u)); }
    // ... and the lane that holds what belongs to it (SLAM_ASSOC_NONE reads some lane; get() says NaN then)
    static __device__ __forceinline__ int lane_of(unsigned k) { return (int)(k & 63u); }
    __device__ __forceinline__ void get(unsigned l, bool in, float& vx, float& vy) const
    {
        const float nan = __uint_as_float(0x7fc00000u);
        const unsigned k = entry(l, in);
        const float dx = __shfl(detx, lane_of(k), 64), dy = __shfl(dety, lane_of(k), 64);
        const bool has = k < 64u;   // SLAM_ASSOC_NONE, and any value that is no detection
        vx = has ? dx : nan;
        vy = has ? dy : nan;
    }
};

template <class NOISE, class OBS> struct EkfRowLane {   // per-wavefront constants of one particle
    typedef NOISE Noise;
    // source row and destination row (p.rout) as buffer resources (wave-uniform descriptors in SGPRs): an access is
    // "descriptor + 32-bit lane offset + scalar plane offset", no 64-bit vector arithmetic for loads or stores
    __amdgpu_buffer_rsrc_t rin;
    EkfPose p;
    int pl;   // plane stride in bytes
    unsigned L;
    NOISE noise;
    OBS obs;
};
typedef EkfRowLane<EkfNoiseIso, EkfObsFrame> EkfLane;   // the grouped form's row tails (ekf_group_body.h)

// NB batches of 128 landmarks starting at lb: all loads first, then the arithmetic, then the stores.  A lane owns
// landmarks l and l + 64 of each batch, so every access is one 256-byte dword access per wavefront (8-byte
// accesses, a lane owning neighbours, were measured ~20 % slower whenever the source rows come out of L2).
// FULL: every lane's landmarks lie inside the row (lb + 128*NB <= plane_stride) and the update is out of place,
// so nothing is predicated; landmarks at or beyond L (row padding) then simply count as "not observed" and their
// padding values are copied along.  !FULL: the general form (row tails, in-place updates).
// W: an EkfRowLane — the wavefront's constants, its arithmetic (W::noise) and where its observations come from (W::obs).
template <int NB, bool FULL, bool COPY, class W>
__device__ __forceinline__ void ekf_batches(const W& w, unsigned lb, unsigned lane, v2f& acc)
{
    const float nan = __uint_as_float(0x7fc00000u);
    v2f m[NB][5], zx[NB], zy[NB];
    typename W::Noise::Aux aux[NB];
    unsigned off[NB][2];
    bool obs[NB][2], use[NB][2];
#pragma unroll
    for (int g = 0; g < NB; ++g)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = lb + (unsigned)g * 128u + 64u * t + lane;
            const bool in = l < w.L;
            off[g][t] = ((FULL || in) ? l : 0u) * 4u;
            float vx, vy;
            w.obs.get(l, in, vx, vy);
            w.noise.fetch(w.obs, l, in, t, aux[g]);
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
                    for (int p = 0; p < 5; ++p) row_store(w.p.rout, off[g][t], p * w.pl, m[g][p][t]);
                }
            continue;
        }
        v2f r0, r1, r2, r3, r4, ll;
        w.noise.update(w.p, mx, my, pxx, pxy, pyy, zx[g], zy[g], aux[g], obs[g][0], obs[g][1], r0, r1, r2, r3, r4, ll);
#pragma unroll
        for (int t = 0; t < 2; ++t)
            if (FULL || use[g][t]) {
                row_store(w.p.rout, off[g][t], 0 * w.pl, r0[t]);
                row_store(w.p.rout, off[g][t], 1 * w.pl, r1[t]);
                row_store(w.p.rout, off[g][t], 2 * w.pl, r2[t]);
                row_store(w.p.rout, off[g][t], 3 * w.pl, r3[t]);
                row_store(w.p.rout, off[g][t], 4 * w.pl, r4[t]);
            }
        acc = acc + ll;
    }
}

// One particle's whole row, NB batches per pass of the fast path (ekf_update_kernel) -> its log-likelihood,
// in every lane.  room: the plane stride in floats.
template <int NB, bool COPY, class W>
__device__ __forceinline__ float ekf_row_walk(const W& w, unsigned room, unsigned lane)
{
    v2f acc = bc2(0.0f);   // lane j: .x = accumulator j, .y = accumulator j + 64 of the spec (landmark l -> l mod 128)
    unsigned lb = 0;
    if (COPY) {   // whole batches that fit into the row, padding included: nothing predicated
        for (; lb < w.L && lb + 128u * NB <= room; lb += 128u * NB) ekf_batches<NB, true, COPY>(w, lb, lane, acc);
        if (NB > 1)
            for (; lb < w.L && lb + 128u <= room; lb += 128u) ekf_batches<1, true, COPY>(w, lb, lane, acc);
    }
    // the general form (row tails; in-place updates).  In place only observed landmarks are touched, so a wavefront's
    // time is round trips, not bytes: NB batches go through one round trip together (batches beyond L load nothing).
    constexpr int NBT = COPY ? 1 : NB;
    for (; lb < w.L; lb += 128u * NBT) ekf_batches<NBT, false, COPY>(w, lb, lane, acc);
    return wave_xor_tree_sum(acc[0] + acc[1]);
}

}  // namespace slam
