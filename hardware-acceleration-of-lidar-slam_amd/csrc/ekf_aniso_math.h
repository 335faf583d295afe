// ekf_aniso_math.h — the arithmetic of ONE landmark update with a full 2x2 measurement covariance in the SENSOR frame
// (S = H P H^T + Q; DESIGN.md section 7, "General measurement covariance"; specification:
// tests/_aniso_spec.py).  ekf_math.h is the case Q = q I; this header is the general one and shares its reciprocal, its
// logarithm and its conventions.  T = float or v2f; every multiply and add is rounded separately, in this order.
//
// Q = [[qxx, qxy], [qxy, qyy]], H^T = [[c, s], [-s, c]] (the convention of ekf_first_sighting).  In the world frame the noise is
//     R_w = H^T Q H,
// which depends on the particle's heading and on nothing else: once per particle.  With S = P + R_w,
//     P'  = R_w S^-1 P = (det P * R_w + det R_w * P) / det S,      mu' = w - R_w S^-1 d,
// (for 2x2 symmetric A, B: A (A + B)^-1 B = (det B * A + det A * B) / det (A + B)) — the cancellation-free form of ekf_math.h:
// no gain matrix, no (I - W) P.  det R_w = det Q exactly in real arithmetic, so it comes from the inputs (detq, once per
// session) and not from the rounded r**.
#pragma once

#include "ekf_math.h"
#include "kernels.h"

namespace slam {

// R_w = H^T Q H of one particle (heading sine s / cosine c)
__device__ __forceinline__ void ekf_aniso_world_noise(const EkfAnisoCov& q, float s, float c, float& rxx, float& rxy, float& ryy)
{
    const float a0 = c * q.qxx + s * q.qxy, a1 = c * q.qxy + s * q.qyy;
    const float b0 = c * q.qxy - s * q.qxx, b1 = c * q.qyy - s * q.qxy;
    rxx = a0 * c + a1 * s;
    rxy = a1 * c - a0 * s;
    ryy = b1 * c - b0 * s;
}

// ... of a Q that differs between the components of T (a covariance per detection: ekf_aniso_lane.h, EkfNoiseDet); the same
// operations in the same order
template <class T> __device__ __forceinline__ void ekf_aniso_world_noise(T qxx, T qxy, T qyy, T s, T c, T& rxx, T& rxy, T& ryy)
{
    const T a0 = c * qxx + s * qxy, a1 = c * qxy + s * qyy;
    const T b0 = c * qxy - s * qxx, b1 = c * qyy - s * qxy;
    rxx = a0 * c + a1 * s;
    rxy = a1 * c - a0 * s;
    ryy = b1 * c - b0 * s;
}

// prior (mx, my, pxx, pxy, pyy), observation (zx, zy) in the sensor frame, pose (px, py, heading sine s / cosine c), the
// particle's R_w (rxx, rxy, ryy) and det Q.  What the update of a landmark seen before gives (o0 .. o4, ll) and the observed
// point in the world frame (f0, f1: what a first sighting stores, with P = R_w and no term); the caller selects as for
// ekf_update_one.
template <class T>
__device__ __forceinline__ EkfResult<T> ekf_aniso_update_one(T mx, T my, T pxx, T pxy, T pyy, T zx, T zy, T s, T c, T px, T py, T rxx,
                                                             T rxy, T ryy, T detq)
{
    EkfResult<T> r;
    const T wx = px + (c * zx + s * zy);
    const T wy = py + (c * zy - s * zx);
    const T dx = wx - mx, dy = wy - my;
    const T a = pxx + rxx, b = pxy + rxy, cc = pyy + ryy;
    const T det = a * cc - b * b;
    const T idet = ekf_rcp(det);
    const T i00 = cc * idet, i01 = -b * idet, i11 = a * idet;               // S^-1
    const T t0 = i00 * dx + i01 * dy, t1 = i01 * dx + i11 * dy;             // S^-1 d
    r.o0 = wx - (rxx * t0 + rxy * t1);
    r.o1 = wy - (rxy * t0 + ryy * t1);
    const T detp = pxx * pyy - pxy * pxy;
    r.o2 = idet * (detp * rxx + detq * pxx);                                // R_w S^-1 P
    r.o3 = idet * (detp * rxy + detq * pxy);
    r.o4 = idet * (detp * ryy + detq * pyy);
    const T maha = dx * t0 + dy * t1;
    const T hl = ekf_splat<T>(0.5f) * ekf_log(det);
    r.ll = ((ekf_splat<T>(0.0f) - ekf_splat<T>(0.5f) * maha) - hl) - ekf_splat<T>(1.8378770664f);
    r.f0 = wx;   // the same expression as ekf_first_sighting
    r.f1 = wy;
    return r;
}

}  // namespace slam
