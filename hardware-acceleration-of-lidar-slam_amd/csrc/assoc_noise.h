// assoc_noise.h — the measurement noise of one particle as an associating kernel sees it (associate_body of assoc_kernels.hip,
// localise_particle of localise_kernels.hip): one policy per noise form, each giving S^-1 = (P + noise)^-1 of the two landmarks of
// a lane — step b of the matching, whose other steps are match_body.h — with the operations, and the reciprocal, of the landmark
// update under that form.  One copy of the arithmetic for every kernel that gates and matches.
//
// A policy is constructed from (its parameters, sine, cosine of the particle's heading), says in kPerDetection whether S^-1 is
// formed once per landmark — inverse(pxx, pxy, pyy) — or per (landmark, detection) pair — inverse(pxx, pxy, pyy, k) — and returns it
// in EkfShared's i00 / i01 / i11.  (A fourth policy of this shape, the inverse read from a prepared map, is LocNoisePrepared of
// localise_kernels.hip.)
#pragma once

#include "ekf_aniso_math.h"
#include "ekf_wave.h"

namespace slam {

struct AssocNoiseIso {   // q I: ekf_det_terms without the logarithm, then ekf_shared_from
    static constexpr bool kPerDetection = false;
    v2f q;
    __device__ __forceinline__ AssocNoiseIso(float meas_var, float, float) : q(bc2(meas_var)) {}
    __device__ __forceinline__ EkfShared<v2f> inverse(v2f pxx, v2f pxy, v2f pyy) const
    {
        const v2f aa = pxx + q, cc = pyy + q;
        const v2f det = aa * cc - pxy * pxy;
        return ekf_shared_from<v2f, false>(pxx, pxy, pyy, q, ekf_rcp(det), bc2(0.0f));
    }
};
struct AssocNoiseAniso {   // R_w = H^T Q H of the particle's heading: the operations of ekf_aniso_update_one, the update's own reciprocal
    static constexpr bool kPerDetection = false;
    float rxx, rxy, ryy;   // wave-uniform, held in scalar registers
    __device__ __forceinline__ AssocNoiseAniso(float xx, float xy, float yy) : rxx(xx), rxy(xy), ryy(yy) {}   // (wave-uniform values)
    __device__ __forceinline__ AssocNoiseAniso(const EkfAnisoCov& q, float s, float c)
    {
        float xx, xy, yy;
        ekf_aniso_world_noise(q, s, c, xx, xy, yy);
        rxx = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xx)));
        rxy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(xy)));
        ryy = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(yy)));
    }
    __device__ __forceinline__ EkfShared<v2f> inverse(v2f pxx, v2f pxy, v2f pyy) const
    {
        EkfShared<v2f> h;   // (only S^-1 is filled in)
        const v2f a = pxx + bc2(rxx), b = pxy + bc2(rxy), cc = pyy + bc2(ryy);
        const v2f det = a * cc - b * b;
        const v2f idet = ekf_rcp(det);
        h.i00 = cc * idet;
        h.i01 = -b * idet;
        h.i11 = a * idet;
        return h;
    }
};
struct AssocNoiseDet {   // R_w(k) = H^T Q_k H: AssocNoiseAniso per detection, S^-1 per (landmark, detection) pair
    static constexpr bool kPerDetection = true;
    float rxx, rxy, ryy;   // lane k: R_w of detection k (lanes from ndet on: of the identity, never read)
    __device__ __forceinline__ AssocNoiseDet(const DetCovArgs& q, float s, float c)
    {
        const int lane = (int)(threadIdx.x & 63u);
        const float qxx = lane < q.ndet ? q.qxx[lane] : 1.0f, qxy = lane < q.ndet ? q.qxy[lane] : 0.0f, qyy = lane < q.ndet ? q.qyy[lane] : 1.0f;
        ekf_aniso_world_noise<float>(qxx, qxy, qyy, s, c, rxx, rxy, ryy);
    }
    __device__ __forceinline__ EkfShared<v2f> inverse(v2f pxx, v2f pxy, v2f pyy, unsigned k) const
    {
        const AssocNoiseAniso one(lane_value(rxx, (int)k), lane_value(rxy, (int)k), lane_value(ryy, (int)k));
        return one.inverse(pxx, pxy, pyy);
    }
};

}  // namespace slam
