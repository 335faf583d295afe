// engine_fov.hip — the field of view of the existence evidence behind the C ABI (fov_kernels.hip): the bound of an angle, and the
// evidence stage with the arc test, with line of sight (the engine's table: engine_sight.hip) or without.

#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "engine_internal.h"
#include "evidence_common.h"

using namespace slam;

extern "C" {

float slam_fov_bound(float angle)
{
    float p;
    (void)diamond_angle(cosf(angle), sinf(angle), p);   // (a NaN or infinite angle has no direction: 0)
    return p;
}

int slam_landmark_evidence_fov_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                                   const float* d_y, const float* d_th, const int32_t* d_anc, int n, const uint8_t* d_assoc,
                                   int assoc_stride, const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax,
                                   float view_range, float margin, float lo, float hi, int use_sight, int32_t* d_stats, int32_t* d_spared,
                                   int32_t* d_outside)
{
    return slam_landmark_evidence_fov_missed_dev(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, d_assoc, assoc_stride,
                                                 d_ev_in, d_ev_out, ev_stride, hit, miss, cmax, view_range, margin, lo, hi, use_sight, d_stats,
                                                 d_spared, d_outside, nullptr);
}

int slam_landmark_evidence_fov_missed_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                                          const float* d_y, const float* d_th, const int32_t* d_anc, int n, const uint8_t* d_assoc,
                                          int assoc_stride, const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss,
                                          int cmax, float view_range, float margin, float lo, float hi, int use_sight, int32_t* d_stats,
                                          int32_t* d_spared, int32_t* d_outside, int32_t* d_missed)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    const float big = std::numeric_limits<float>::max();
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || ev_stride < nlandmarks || hit < 1 || hit > 255 || miss < 1 || miss > 255 || cmax < 1 || cmax > 255 ||
        !(view_range > 0.0f && view_range <= big) || (use_sight && !(margin > 0.0f && margin <= big)) ||   // (NaN fails every comparison)
        !fov_bounds_ok(lo, hi) || !d_map || !d_x || !d_y || !d_th || !d_assoc || !d_ev_in || !d_ev_out || (d_anc && d_ev_in == d_ev_out))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0 || (use_sight && e->sight_bins == 0)) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    EvidenceArgs a;
    a.map = d_map;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x = d_x;
    a.y = d_y;
    a.anc = d_anc;
    a.n = n;
    a.assoc = d_assoc;
    a.assoc_stride = assoc_stride;
    a.ndet = e->ndet;
    a.ev_in = d_ev_in;
    a.ev_out = d_ev_out;
    a.ev_stride = ev_stride;
    a.hit = hit;
    a.miss = miss;
    a.cmax = cmax;
    a.range2 = view_range * view_range;   // one float32 product (-ffp-contract=off)
    a.stats = d_stats;
    a.missed = d_missed;
    a.xcd_chunk = 0;
    const SightArgs sg{ d_th, use_sight ? e->sight_buf.as<float>() : nullptr, use_sight ? e->sight_bins : 0, use_sight ? margin : 0.0f, d_spared };
    const FovArgs fv{ lo, hi, d_outside };
    SLAM_HIP_TRY(e, launch_landmark_evidence_fov(e->stream, a, sg, fv, e->prof_next(SLAM_PROF_PAGES)));
    e->fov_launches++;
    return SLAM_OK;
}

int slam_fov_counts(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->fov_launches;
    return SLAM_OK;
}

}  // extern "C"
