// ekf_aniso_lane.h — the lane type of the row walk (ekf_row_body.h) under a full 2x2 measurement covariance: what
// ekf_aniso_kernel (ekf_aniso_kernels.hip) and the update under a per-particle table (assoc_kernels.hip) both walk their rows with.
#pragma once

#include "ekf_aniso_math.h"
#include "ekf_row_body.h"

namespace slam {

struct EkfAnisoLane {   // per-wavefront constants of one particle (EkfLane with R_w and det Q in the place of q)
    __amdgpu_buffer_rsrc_t rin;
    EkfPose p;
    int pl;   // plane stride in bytes
    const gchar *ozx, *ozy;
    unsigned L;
    v2f rxx, rxy, ryy, detq;
    __device__ __forceinline__ void update(v2f mx, v2f my, v2f pxx, v2f pxy, v2f pyy, v2f zx, v2f zy, bool ob0, bool ob1, v2f& r0, v2f& r1,
                                           v2f& r2, v2f& r3, v2f& r4, v2f& ll) const
    {
        const EkfResult<v2f> u = ekf_aniso_update_one<v2f>(mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, detq);
        r0 = u.o0; r1 = u.o1; r2 = u.o2; r3 = u.o3; r4 = u.o4; ll = u.ll;
        ekf_select(r0, r1, r2, r3, r4, ll, mx, my, pxx, pxy, pyy, zx, zy, p.s, p.c, p.px, p.py, rxx, rxy, ryy, ob0, ob1);
    }
};

}  // namespace slam
