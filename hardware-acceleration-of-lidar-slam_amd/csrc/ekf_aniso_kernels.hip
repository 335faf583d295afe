// ekf_aniso_kernels.hip — the landmark update with a full 2x2 measurement covariance in the sensor frame (SURVEY.md row A10;
// the arithmetic: ekf_aniso_math.h; specification: tests/_aniso_spec.py).  The world-frame noise R_w = H^T Q H depends on the
// particle's heading, so the posterior covariance is per particle again: only the row layout stores that, and this is a form
// of the row update alone — one wavefront per particle walking its row (ekf_row_body.h: ekf_row_walk, the walk of
// ekf_update_kernel), out of place through a gather index or in place.  What differs from ekf_update_kernel is the arithmetic
// per landmark and what a first sighting stores (P = R_w); R_w and the pose are wave-uniform.  No grouped form, no
// observation-list form, no fused front.

#include "ekf_aniso_lane.h"

namespace slam {

namespace {

// NB: batches of 128 landmarks per pass of the fast path.  COPY: out of place.
template <int NB, bool COPY>
__global__ __launch_bounds__(kEkfWaves * 64) void ekf_aniso_kernel(EkfArgs a, EkfAnisoCov q)
{
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i = xcd_block(a.xcd_chunk) * kEkfWaves + wave;
    if (i >= a.n) return;
    const int src = a.anc ? a.anc[i] : i;
    float st_, ct_, rxx, rxy, ryy;
    det_sincosf(a.th[i], st_, ct_);
    ekf_aniso_world_noise(q, st_, ct_, rxx, rxy, ryy);
    EkfAnisoLane w;
    const int row_bytes = __builtin_amdgcn_readfirstlane(5 * a.plane_stride * 4);
    w.rin = row_rsrc(a.map_in, src, a.row_stride, row_bytes);
    w.p.rout = row_rsrc(a.map_out, i, a.row_stride, row_bytes);
    w.pl = __builtin_amdgcn_readfirstlane(a.plane_stride * 4);
    w.ozx = uniform_gptr(a.obs_zx);
    w.ozy = uniform_gptr(a.obs_zy);
    w.L = (unsigned)a.nlandmarks;
    w.p.s = bc2(st_); w.p.c = bc2(ct_); w.p.px = bc2(a.x[i]); w.p.py = bc2(a.y[i]);
    w.rxx = bc2(rxx); w.rxy = bc2(rxy); w.ryy = bc2(ryy); w.detq = bc2(q.detq);

    const float total = ekf_row_walk<NB, COPY>(w, (unsigned)a.plane_stride, lane);
    if (lane == 0) store_loglik(a, i, total);
}

}  // namespace

hipError_t launch_ekf_aniso(hipStream_t stream, const EkfArgs& a_in, const EkfAnisoCov& q, const EventPair* ev)
{
    if (a_in.n <= 0) return hipSuccess;
    if (a_in.cov) return hipErrorInvalidValue;   // rows only
    EkfArgs a = a_in;
    const bool copy = a.map_in != a.map_out;   // in place: rows without an observation stay as they are
    // batches per pass: those of ekf_update_kernel (launch_ekf_update, its form 0) at the same shapes
    void (*kernel)(EkfArgs, EkfAnisoCov);
    if (!copy) kernel = a.nlandmarks > 128 ? ekf_aniso_kernel<4, false> : ekf_aniso_kernel<1, false>;
    else kernel = a.nlandmarks > 128 ? ekf_aniso_kernel<2, true> : ekf_aniso_kernel<1, true>;
    const int blocks = xcd_grid(a.n, kEkfWaves, a.xcd_chunk);
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, 0, stream>>>(a, q);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
