// ekf_aniso_lane.h — the noise policies of the row walk (ekf_row_body.h: EkfRowLane) under a full 2x2 measurement covariance in the
// sensor frame (the arithmetic: ekf_aniso_math.h; specification: tests/_aniso_spec.py).  The world-frame noise
// R_w = H^T Q H depends on the particle's heading, so the posterior covariance is per particle again: only the row layout stores
// that, and this is a form of the one-wavefront-per-particle row update alone (ekf_update_kernel of ekf_kernels.hip) — no grouped
// form, no observation-list form, no fused front.  R_w and the pose are wave-uniform.
#pragma once

#include "ekf_aniso_math.h"
#include "ekf_row_body.h"

namespace slam {

struct EkfNoiseAniso {   // EkfNoiseIso with R_w and det Q in the place of q (a.meas_var is not read; a first sighting stores P = R_w)
    typedef EkfAnisoCov Args;
    struct Aux {};
    v2f rxx, rxy, ryy, detq;
    __device__ __forceinline__ void init(const EkfArgs& a, const Args& q, float s, float c)
    {
        float xx, xy, yy;
        ekf_aniso_world_noise(q, s, c, xx, xy, yy);
        rxx = bc2(xx); rxy = bc2(xy); ryy = bc2(yy); detq = bc2(q.detq);
    }
    template <class OBS> __device__ __forceinline__ void fetch(const OBS&, unsigned l, bool in, int t, Aux&) const {}
    __device__ __forceinline__ void update(const EkfPose& p, v2f mx, v2f my, v2f pxx, v2f pxy, v2f pyy, v2f zx, v2f zy, const Aux&, bool ob0, bool ob1,
                                           v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll) const
    {
        const EkfResult<v2f> u = ekf_aniso_update_one<v2f>(mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, detq);
        r0 = u.o0; r1 = u.o1; r2 = u.o2; r3 = u.o3; r4 = u.o4; ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, ob0, ob1);
    }
};

// A covariance per detection (specification: tests/_assoc_detcov_spec.py; with EkfObsTable only): lane k of the wavefront holds
// Q_k beside detection k, the lane that fetched its landmark's z through the table byte fetches that detection's Q the same
// way (three more lane reads, no further trip to memory), and R_w = H^T Q_k H and det Q_k are formed per lane pair — the
// operations of ekf_aniso_world_noise and ekf_aniso_cov on v2f.  A landmark without a detection reads some lane's Q (lanes from
// ndet on hold the identity) and ekf_select discards what comes of it.
struct EkfNoiseDet {
    typedef DetCovArgs Args;
    struct Aux {
        v2f qxx, qxy, qyy;
    };
    float qxx, qxy, qyy;   // THIS lane's detection's Q
    __device__ __forceinline__ void init(const EkfArgs& a, const Args& q, float s, float c)
    {
        const int lane = (int)(threadIdx.x & 63u);
        qxx = lane < q.ndet ? q.qxx[lane] : 1.0f;
        qxy = lane < q.ndet ? q.qxy[lane] : 0.0f;
        qyy = lane < q.ndet ? q.qyy[lane] : 1.0f;
    }
    __device__ __forceinline__ void fetch(const EkfObsTable& obs, unsigned l, bool in, int t, Aux& x) const
    {
        const int k = EkfObsTable::lane_of(obs.entry(l, in));   // where get() finds z, Q lies beside it
        x.qxx[t] = __shfl(qxx, k, 64);
        x.qxy[t] = __shfl(qxy, k, 64);
        x.qyy[t] = __shfl(qyy, k, 64);
    }
    __device__ __forceinline__ void update(const EkfPose& p, v2f mx, v2f my, v2f pxx, v2f pxy, v2f pyy, v2f zx, v2f zy, const Aux& x, bool ob0,
                                           bool ob1, v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll) const
    {
        v2f rxx, rxy, ryy;
        ekf_aniso_world_noise<v2f>(x.qxx, x.qxy, x.qyy, p.s, p.c, rxx, rxy, ryy);
        const v2f t0 = x.qxx * x.qyy, t1 = x.qxy * x.qxy;
        const v2f detq = t0 - t1;
        const EkfResult<v2f> u = ekf_aniso_update_one<v2f>(mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, detq);
        r0 = u.o0; r1 = u.o1; r2 = u.o2; r3 = u.o3; r4 = u.o4; ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, ob0, ob1);
    }
};

}  // namespace slam
