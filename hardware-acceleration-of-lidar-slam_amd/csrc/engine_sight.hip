// engine_sight.hip — line of sight for the existence evidence behind the C ABI (sight_kernels.hip): the sight table of the
// engine's current scan, and the evidence stage that reads it.  The evidence stage without it: engine_assoc.hip.

#include <hip/hip_runtime.h>

#include <limits>

#include "engine_internal.h"

using namespace slam;

extern "C" {

int slam_sight_table_dev(slam_engine* e, int bins)
{
    SLAM_ENTER(e);
    if (!sight_bins_ok(bins)) return SLAM_ERR_INVALID_ARG;
    if (e->nbeams < 0) return SLAM_ERR_NOT_READY;
    if (!e->sight_buf.p) SLAM_HIP_TRY(e, e->sight_buf.ensure(sizeof(float) * kSightMaxBins));
    SLAM_HIP_TRY(e, launch_sight_table(e->stream, e->d_bx, e->d_by, e->nbeams, bins, e->sight_buf.as<float>(), e->prof_next(SLAM_PROF_PAGES)));
    e->sight_bins = bins;
    e->sight_launches[0]++;
    return SLAM_OK;
}

int slam_sight_table_get_host(slam_engine* e, float* t, int32_t* bins)
{
    SLAM_ENTER(e);
    if (!t || !bins) return SLAM_ERR_INVALID_ARG;
    if (e->sight_bins == 0) return SLAM_ERR_NOT_READY;
    SLAM_HIP_TRY(e, hipMemcpyAsync(t, e->sight_buf.as<float>(), sizeof(float) * (size_t)e->sight_bins, hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    *bins = e->sight_bins;
    return SLAM_OK;
}

int slam_landmark_evidence_sight_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                                     const float* d_y, const float* d_th, const int32_t* d_anc, int n, const uint8_t* d_assoc,
                                     int assoc_stride, const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax,
                                     float view_range, float margin, int32_t* d_stats, int32_t* d_spared)
{
    return slam_landmark_evidence_sight_missed_dev(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, d_assoc,
                                                   assoc_stride, d_ev_in, d_ev_out, ev_stride, hit, miss, cmax, view_range, margin, d_stats,
                                                   d_spared, nullptr);
}

int slam_landmark_evidence_sight_missed_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                            const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                            const uint8_t* d_assoc, int assoc_stride, const uint8_t* d_ev_in, uint8_t* d_ev_out,
                                            int ev_stride, int hit, int miss, int cmax, float view_range, float margin, int32_t* d_stats,
                                            int32_t* d_spared, int32_t* d_missed)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    const float big = std::numeric_limits<float>::max();
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || ev_stride < nlandmarks || hit < 1 || hit > 255 || miss < 1 || miss > 255 || cmax < 1 || cmax > 255 ||
        !(view_range > 0.0f && view_range <= big) || !(margin > 0.0f && margin <= big) ||   // (NaN fails every comparison)
        !d_map || !d_x || !d_y || !d_th || !d_assoc || !d_ev_in || !d_ev_out || (d_anc && d_ev_in == d_ev_out))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0 || e->sight_bins == 0) return SLAM_ERR_NOT_READY;
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
    const SightArgs sg{ d_th, e->sight_buf.as<float>(), e->sight_bins, margin, d_spared };
    SLAM_HIP_TRY(e, launch_landmark_evidence_sight(e->stream, a, sg, e->prof_next(SLAM_PROF_PAGES)));
    e->sight_launches[1]++;
    return SLAM_OK;
}

int slam_sight_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->sight_launches[0];
    counts[1] = e->sight_launches[1];
    return SLAM_OK;
}

}  // extern "C"
