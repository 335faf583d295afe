// engine_merge.hip — merging duplicate landmarks behind the C ABI (merge_kernels.hip): the stage on rows, in place, behind the
// frame's associating update and its evidence stage, and its launch counter.

#include <hip/hip_runtime.h>

#include <limits>

#include "engine_internal.h"

using namespace slam;

extern "C" {

int slam_landmark_merge_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, int n, const uint8_t* d_assoc,
                            int assoc_stride, uint8_t* d_ev, int ev_stride, int cmax, float merge_gate, int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    const float big = std::numeric_limits<float>::max();
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || !(merge_gate > 0.0f && merge_gate <= big) ||   // (NaN fails every comparison)
        (d_ev && (ev_stride < nlandmarks || cmax < 1 || cmax > 255)) || !d_map || !d_assoc)
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    MergeArgs a;
    a.map = d_map;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.n = n;
    a.assoc = d_assoc;
    a.assoc_stride = assoc_stride;
    a.ndet = e->ndet;
    a.ev = d_ev;
    a.ev_stride = d_ev ? ev_stride : 0;
    a.cmax = d_ev ? cmax : 0;
    a.gate = merge_gate;
    a.stats = d_stats;
    a.xcd_chunk = 0;
    SLAM_HIP_TRY(e, launch_landmark_merge(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->merge_launches++;
    return SLAM_OK;
}

int slam_merge_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->merge_launches;
    return SLAM_OK;
}

}  // extern "C"
