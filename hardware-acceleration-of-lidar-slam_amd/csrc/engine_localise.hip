// engine_localise.hip — localisation in a known landmark map behind the C ABI (localise_kernels.hip): the prepared map, made once
// per map, and the stage of a frame — the engine's current detections against that map, per particle, into the engine's
// log-likelihood buffer (what slam_logweight_ekf_dev consumes) or the caller's.  Under the detections' own covariances
// (slam_localise_detcov_dev) nothing is prepared: the stage reads the map as it was given.  The _miss entry points are the same
// path with a view: the launch also counts the landmarks in view that no detection matched.

#include <hip/hip_runtime.h>

#include <limits>

#include "engine_internal.h"

using namespace slam;

extern "C" {

int slam_known_map_prepare_dev(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, float meas_var, float* d_prepared)
{
    SLAM_ENTER(e);
    if (!d_map || !d_prepared || nlandmarks < 1 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || !(meas_var > 0.0f)) return SLAM_ERR_INVALID_ARG;
    const KnownMapArgs a{ d_map, plane_stride, nlandmarks, meas_var, d_prepared };
    SLAM_HIP_TRY(e, launch_known_map_prepare(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->localise_launches[0]++;
    return SLAM_OK;
}

// what the _miss entry points add to the other two
struct LocaliseMiss {
    const slam_localise_view* view;
    int32_t *d_missed, *d_spared, *d_outside;
};

// the one checked path of the four entry points.  detcov: d_map is the map as it was given, the engine's detections must carry
// their covariances, and the launch counts as slam_localise_detcov_dev's; else d_map is the prepared map.  miss: the miss form of
// either, which counts as slam_localise_miss_count's only
static int localise(slam_engine* e, bool detcov, const float* d_map, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                    const float* d_th, int n, float gate, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats, float* d_loglik,
                    const LocaliseMiss* miss = nullptr)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (n < 0 || nlandmarks < 1 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || (d_assoc && assoc_stride < nlandmarks) ||
        !(gate > 0.0f && gate <= std::numeric_limits<float>::max()) || !d_map || (n > 0 && (!d_x || !d_y || !d_th || !d_stats)))
        return SLAM_ERR_INVALID_ARG;
    const float big = std::numeric_limits<float>::max();
    const slam_localise_view* vw = miss ? miss->view : nullptr;
    if (miss && (!vw || !miss->d_missed || !(vw->view_range > 0.0f && vw->view_range <= big) || !fov_bounds_ok(vw->lo, vw->hi) ||   // (NaN fails every comparison)
                 (vw->sight && !(vw->margin > 0.0f && vw->margin <= big))))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0 || (detcov && !e->det_has_cov) || (miss && vw->sight && e->sight_bins == 0)) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    if (!d_loglik) SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    LocaliseArgs a;
    a.map = d_map;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x = d_x;
    a.y = d_y;
    a.th = d_th;
    a.n = n;
    a.det_zx = e->d_det_zx;
    a.det_zy = e->d_det_zy;
    a.ndet = e->ndet;
    a.gate = gate;
    a.assoc = d_assoc;
    a.assoc_stride = assoc_stride;
    a.stats = d_stats;
    a.loglik = d_loglik ? d_loglik : e->ll_buf.as<float>();
    const DetCovArgs dq{ e->d_det_qxx, e->d_det_qxy, e->d_det_qyy, e->ndet };
    LocMissArgs v{};
    if (miss) {
        const bool sight = vw->sight != 0;
        v.range2 = vw->view_range * vw->view_range;   // one float32 product (-ffp-contract=off)
        v.fov = !(vw->lo == 0.0f && vw->hi == 4.0f);  // the whole circle: every direction passes the arc test, which is skipped
        v.lo = vw->lo;
        v.hi = vw->hi;
        v.table = sight ? e->sight_buf.as<float>() : nullptr;
        v.bins = sight ? e->sight_bins : 0;
        v.margin = sight ? vw->margin : 0.0f;
        v.missed = miss->d_missed;
        v.spared = miss->d_spared;
        v.outside = miss->d_outside;
    }
    SLAM_HIP_TRY(e, launch_localise(e->stream, a, detcov ? &dq : nullptr, miss ? &v : nullptr, e->prof_next(SLAM_PROF_PAGES)));
    if (!d_loglik) e->ll_n = n;
    (miss ? e->localise_miss_launches : detcov ? e->localise_detcov_launches : e->localise_launches[1])++;   // each form in its own counter only
    return SLAM_OK;
}

int slam_localise_dev(slam_engine* e, const float* d_prepared, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                      const float* d_th, int n, float gate, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats, float* d_loglik)
{
    return localise(e, false, d_prepared, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik);
}

int slam_localise_detcov_dev(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                             const float* d_th, int n, float gate, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats, float* d_loglik)
{
    return localise(e, true, d_map, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik);
}

int slam_localise_miss_dev(slam_engine* e, const float* d_prepared, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                           const float* d_th, int n, float gate, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats, float* d_loglik,
                           const slam_localise_view* view, int32_t* d_missed, int32_t* d_spared, int32_t* d_outside)
{
    const LocaliseMiss miss{ view, d_missed, d_spared, d_outside };
    return localise(e, false, d_prepared, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik, &miss);
}

int slam_localise_detcov_miss_dev(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                                  const float* d_th, int n, float gate, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats, float* d_loglik,
                                  const slam_localise_view* view, int32_t* d_missed, int32_t* d_spared, int32_t* d_outside)
{
    const LocaliseMiss miss{ view, d_missed, d_spared, d_outside };
    return localise(e, true, d_map, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, d_assoc, assoc_stride, d_stats, d_loglik, &miss);
}

int slam_localise_miss_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->localise_miss_launches;
    return SLAM_OK;
}

int slam_localise_detcov_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->localise_detcov_launches;
    return SLAM_OK;
}

int slam_localise_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->localise_launches[0];
    counts[1] = e->localise_launches[1];
    return SLAM_OK;
}

}  // extern "C"
