// engine_evidence.hip — the landmarks' existence evidence behind the C ABI (evidence_kernels.hip, sight_kernels.hip): the evidence
// stage in every form — plain, with line of sight, with a field of view — as ONE path (slam_engine_evidence) behind its six entry
// points; the sight table of the engine's current scan, the bound of an angle, init, gather and the counters.

#include <hip/hip_runtime.h>

#include <cmath>
#include <limits>

#include "engine_internal.h"
#include "evidence_common.h"

using namespace slam;

int slam_engine_evidence(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                         const int32_t* d_anc, int n, const uint8_t* d_assoc, int assoc_stride, const uint8_t* d_ev_in, uint8_t* d_ev_out,
                         int ev_stride, int hit, int miss, int cmax, float view_range, int32_t* d_stats, int32_t* d_missed,
                         const slam_evidence_form& form)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    const float big = std::numeric_limits<float>::max();
    const bool directed = form.use_sight || form.fov;   // the landmark's direction in the sensor frame is needed: the headings
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || ev_stride < nlandmarks || hit < 1 || hit > 255 || miss < 1 || miss > 255 || cmax < 1 || cmax > 255 ||
        !(view_range > 0.0f && view_range <= big) || (form.use_sight && !(form.margin > 0.0f && form.margin <= big)) ||   // (NaN fails every comparison)
        (form.fov && !fov_bounds_ok(form.lo, form.hi)) || !d_map || !d_x || !d_y || (directed && !form.d_th) || !d_assoc || !d_ev_in ||
        !d_ev_out || (d_anc && d_ev_in == d_ev_out))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0 || (form.use_sight && e->sight_bins == 0)) return SLAM_ERR_NOT_READY;
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
    const bool sight = form.use_sight;
    const SightArgs sg{ form.d_th, sight ? e->sight_buf.as<float>() : nullptr, sight ? e->sight_bins : 0, sight ? form.margin : 0.0f, form.d_spared };
    const FovArgs fv{ form.lo, form.hi, form.d_outside };
    SLAM_HIP_TRY(e, launch_landmark_evidence(e->stream, a, directed ? &sg : nullptr, form.fov ? &fv : nullptr, e->prof_next(SLAM_PROF_PAGES)));
    (form.fov ? e->fov_launches : sight ? e->sight_launches[1] : e->evidence_launches[0])++;   // each form in its own counter only
    return SLAM_OK;
}

extern "C" {

/* ------------------------------------------------------------------ the stage's six entry points: a form each, one path */

int slam_landmark_evidence_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                               const float* d_y, const int32_t* d_anc, int n, const uint8_t* d_assoc, int assoc_stride,
                               const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax, float view_range,
                               int32_t* d_stats)
{
    return slam_landmark_evidence_missed_dev(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_anc, n, d_assoc, assoc_stride, d_ev_in,
                                             d_ev_out, ev_stride, hit, miss, cmax, view_range, d_stats, nullptr);
}

int slam_landmark_evidence_missed_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                                      const float* d_y, const int32_t* d_anc, int n, const uint8_t* d_assoc, int assoc_stride,
                                      const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax,
                                      float view_range, int32_t* d_stats, int32_t* d_missed)
{
    return slam_engine_evidence(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_anc, n, d_assoc, assoc_stride, d_ev_in, d_ev_out,
                                ev_stride, hit, miss, cmax, view_range, d_stats, d_missed, slam_evidence_form{});
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
    const slam_evidence_form form{ d_th, margin, true, false, 0.0f, 0.0f, d_spared, nullptr };
    return slam_engine_evidence(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_anc, n, d_assoc, assoc_stride, d_ev_in, d_ev_out,
                                ev_stride, hit, miss, cmax, view_range, d_stats, d_missed, form);
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
    const slam_evidence_form form{ d_th, margin, use_sight != 0, true, lo, hi, d_spared, d_outside };
    return slam_engine_evidence(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_anc, n, d_assoc, assoc_stride, d_ev_in, d_ev_out,
                                ev_stride, hit, miss, cmax, view_range, d_stats, d_missed, form);
}

/* ------------------------------------------------------------------ the sight table, the bound of an angle */

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

float slam_fov_bound(float angle)
{
    float p;
    (void)diamond_angle(cosf(angle), sinf(angle), p);   // (a NaN or infinite angle has no direction: 0)
    return p;
}

/* ------------------------------------------------------------------ init, gather, counters */

int slam_evidence_init_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, int nrows,
                           uint8_t* d_ev, int ev_stride, int value)
{
    SLAM_ENTER(e);
    if (nrows < 0 || nlandmarks < 0 || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride || ev_stride < nlandmarks ||
        value < 0 || value > 255 || !d_map || !d_ev)
        return SLAM_ERR_INVALID_ARG;
    if (nrows == 0) return SLAM_OK;
    EvidenceInitArgs a;
    a.map = d_map;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.nrows = nrows;
    a.ev = d_ev;
    a.ev_stride = ev_stride;
    a.value = value;
    a.xcd_chunk = 0;
    SLAM_HIP_TRY(e, launch_evidence_init(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->evidence_launches[1]++;
    return SLAM_OK;
}

int slam_evidence_gather_dev(slam_engine* e, const uint8_t* d_in, uint8_t* d_out, int ev_stride, const int32_t* d_anc, int n)
{
    SLAM_ENTER(e);
    if (n < 0 || ev_stride < 0 || (n > 0 && ev_stride > 0 && (!d_in || !d_out || !d_anc || d_in == d_out))) return SLAM_ERR_INVALID_ARG;
    const ProfScope prof(e, SLAM_PROF_PAGES);
    SLAM_HIP_TRY(e, launch_evidence_gather(e->stream, d_in, d_out, ev_stride, d_anc, n));
    return SLAM_OK;
}

int slam_evidence_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->evidence_launches[0];
    counts[1] = e->evidence_launches[1];
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

int slam_fov_counts(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->fov_launches;
    return SLAM_OK;
}

}  // extern "C"
