// ekf_aniso_lane.h — the noise policy of the row walk (ekf_row_body.h: EkfRowLane) under a full 2x2 measurement covariance in the
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
    v2f rxx, rxy, ryy, detq;
    __device__ __forceinline__ void init(const EkfArgs& a, const Args& q, float s, float c)
    {
        float xx, xy, yy;
        ekf_aniso_world_noise(q, s, c, xx, xy, yy);
        rxx = bc2(xx); rxy = bc2(xy); ryy = bc2(yy); detq = bc2(q.detq);
    }
    __device__ __forceinline__ void update(const EkfPose& p, v2f mx, v2f my, v2f pxx, v2f pxy, v2f pyy, v2f zx, v2f zy, bool ob0, bool ob1,
                                           v2f& r0, v2f& r1, v2f& r2, v2f& r3, v2f& r4, v2f& ll) const
    {
        const EkfResult<v2f> u = ekf_aniso_update_one<v2f>(mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, detq);
        r0 = u.o0; r1 = u.o1; r2 = u.o2; r3 = u.o3; r4 = u.o4; ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, ob0, ob1);
    }
};

}  // namespace slam
