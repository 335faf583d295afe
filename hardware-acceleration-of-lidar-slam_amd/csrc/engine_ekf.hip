// engine_ekf.hip — the landmark side of a particle-filter frame behind the C ABI: motion sample (alone, or with the score of
// the sampled poses), the observation table, the landmark update in every form (in place, out of place, split layout, fused
// with motion + score as the frame's front launch), the switches and counters of those forms, data association (the frame's
// detections, the association stage and the update under a per-particle table, with meas_var * I or a 2x2 Q), the detector that makes the detections from
// the scan, and the landmarks' existence evidence.

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <limits>

#include "engine_internal.h"

using namespace slam;

int slam_engine_resolve_detections(slam_engine* e)
{
    if (!e->det_pending) return SLAM_OK;
    const volatile uint32_t* flag = reinterpret_cast<const volatile uint32_t*>(e->h_det + 1);
    if (int rc = slam_engine_wait_flag(e, nullptr, flag, e->det_seq, "detection count flag")) return rc;
    const int ndet = e->h_det[0];
    if (ndet < 0 || ndet > SLAM_MAX_DETECTIONS) return slam_engine_fail_hip(e, hipErrorUnknown, "detection count");
    e->ndet = ndet;
    e->det_pending = false;
    return SLAM_OK;
}

extern "C" {

/* ------------------------------------------------------------------ particle-filter stages */

int slam_motion_sample_dev(slam_engine* e, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                           const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id,
                           const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame)
{
    SLAM_ENTER(e);
    if (n < 0 || first_id < 0 || !dp || !sigma ||
        (n > 0 && (!d_src_x || !d_src_y || !d_src_th || !d_x || !d_y || !d_th)))
        return SLAM_ERR_INVALID_ARG;
    if (d_anc && (d_src_x == d_x || d_src_y == d_y || d_src_th == d_th)) return SLAM_ERR_INVALID_ARG;   // gather in place
    SLAM_HIP_TRY(e, launch_motion_sample(e->stream, d_src_x, d_src_y, d_src_th, d_anc, d_x, d_y, d_th, n, first_id, dp, sigma,
                                         seed, frame));
    return SLAM_OK;
}

int slam_motion_score_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                          const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id,
                          const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame, float* d_score,
                          int32_t* d_count)
{
    return slam_motion_score_rider_dev(e, slot, d_src_x, d_src_y, d_src_th, d_anc, d_x, d_y, d_th, n, first_id, dp, sigma, seed, frame,
                                       d_score, d_count, nullptr, nullptr);
}

// ... with a paged session's free list in workgroups of the same launch (kernels.h: FreeListRider); *rode = false: the caller
// launches the list by itself
int slam_motion_score_rider_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                                const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id,
                                const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame, float* d_score,
                                int32_t* d_count, const FreeListRider* rider, bool* rode)
{
    SLAM_ENTER(e);
    if (rode) *rode = false;
    if (n < 0 || first_id < 0 || !dp || !sigma ||
        (n > 0 && (!d_src_x || !d_src_y || !d_src_th || !d_x || !d_y || !d_th || !d_score || !d_count)))
        return SLAM_ERR_INVALID_ARG;
    if (d_src_x == d_x || d_src_y == d_y || d_src_th == d_th) return SLAM_ERR_INVALID_ARG;   // several lanes re-read src
    if (int rc = check_score_inputs(e, slot)) return rc;
    MotionIO io{ d_src_x, d_src_y, d_src_th, d_anc, d_x, d_y, d_th, rider ? *rider : FreeListRider() };
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, n, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_motion_score(e->stream, sg, e->d_bx, e->d_by, e->nbeams, io, n, first_id, dp,
                                        sigma, seed, frame, d_score, d_count, e->prof_next(SLAM_PROF_SCORE), rode));
    return SLAM_OK;
}

static bool refine_args_ok(float step_xy, float step_theta, int sweeps)
{
    return sweeps >= 1 && sweeps <= 16 && step_xy >= 0.0f && step_theta >= 0.0f && step_xy <= std::numeric_limits<float>::max() &&
           step_theta <= std::numeric_limits<float>::max();   // (NaN fails every comparison)
}

int slam_refine_poses_dev(slam_engine* e, int slot, float* d_x, float* d_y, float* d_th, int n, float step_xy, float step_theta,
                          int sweeps, float* d_score, int32_t* d_count)
{
    SLAM_ENTER(e);
    if (n < 0 || !refine_args_ok(step_xy, step_theta, sweeps) || (n > 0 && (!d_x || !d_y || !d_th || !d_score || !d_count)))
        return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, n, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_refine_poses(e->stream, sg, e->d_bx, e->d_by, e->nbeams, d_x, d_y, d_th, n, step_xy, step_theta, sweeps,
                                        d_score, d_count, e->prof_next(SLAM_PROF_SCORE)));
    return SLAM_OK;
}

int slam_motion_refine_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                           const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id, const float dp[3],
                           const float sigma[3], uint64_t seed, uint32_t frame, float step_xy, float step_theta, int sweeps,
                           float* d_score, int32_t* d_count)
{
    SLAM_ENTER(e);
    if (n < 0 || first_id < 0 || !dp || !sigma || !refine_args_ok(step_xy, step_theta, sweeps) ||
        (n > 0 && (!d_src_x || !d_src_y || !d_src_th || !d_x || !d_y || !d_th || !d_score || !d_count)))
        return SLAM_ERR_INVALID_ARG;
    if (n > 0 && (d_src_x == d_x || d_src_y == d_y || d_src_th == d_th)) return SLAM_ERR_INVALID_ARG;   // several lanes re-read src
    if (int rc = check_score_inputs(e, slot)) return rc;
    const MotionIO io{ d_src_x, d_src_y, d_src_th, d_anc, d_x, d_y, d_th, FreeListRider() };
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, n, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_motion_refine(e->stream, sg, e->d_bx, e->d_by, e->nbeams, io, n, first_id, dp, sigma, seed, frame, step_xy,
                                         step_theta, sweeps, d_score, d_count, e->prof_next(SLAM_PROF_SCORE)));
    return SLAM_OK;
}

int slam_obs_upload_host(slam_engine* e, const int32_t* landmark_id, const float* zx, const float* zy, int nobs,
                         int nlandmarks)
{
    SLAM_ENTER(e);
    if (nobs < 0 || nlandmarks < 0 || nobs > nlandmarks || (nobs > 0 && (!landmark_id || !zx || !zy)))
        return SLAM_ERR_INVALID_ARG;
    if (nlandmarks > SLAM_MAX_OBS) return SLAM_ERR_CAPACITY;
    // the engine works on a table indexed by landmark: zx[l], zy[l], NaN = no observation of l this frame
    float* h = e->stage_acquire();
    const size_t L = (size_t)nlandmarks;
    float* hx = h;
    float* hy = h + L;
    const float nan = std::numeric_limits<float>::quiet_NaN();
    for (size_t l = 0; l < L; ++l) hx[l] = hy[l] = nan;
    int rc = SLAM_OK;
    for (int k = 0; k < nobs && rc == SLAM_OK; ++k) {
        const int32_t id = landmark_id[k];
        if (id < 0 || id >= nlandmarks || hx[id] == hx[id] || zx[k] != zx[k] || zy[k] != zy[k])
            rc = SLAM_ERR_INVALID_ARG;   // out of range, listed twice, or a NaN measurement
        else {
            hx[id] = zx[k];
            hy[id] = zy[k];
        }
    }
    if (rc != SLAM_OK) {
        (void)e->stage_release(h);   // nothing was queued from this slot
        return rc;
    }
    if (e->obs_buf.cap < 2 * L * 4) {
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));   // a running kernel may still read the old table
        SLAM_HIP_TRY(e, e->obs_buf.ensure(2 * L * 4 > 8 ? 2 * L * 4 : 8));
    }
    if (L > 0) SLAM_HIP_TRY(e, hipMemcpyAsync(e->obs_buf.as<float>(), h, sizeof(float) * 2 * L, hipMemcpyHostToDevice, e->stream));
    SLAM_HIP_TRY(e, e->stage_release(h));
    e->d_obs_zx = e->obs_buf.as<float>();
    e->d_obs_zy = e->obs_buf.as<float>() + L;
    e->obs_nlandmarks = nlandmarks;
    e->obs_list_valid = false;
    e->obs_table_owned = true;
    return SLAM_OK;
}

int slam_obs_set_dev(slam_engine* e, const float* d_zx_by_landmark, const float* d_zy_by_landmark, int nlandmarks)
{
    SLAM_ENTER(e);
    if (nlandmarks < 0 || (nlandmarks > 0 && (!d_zx_by_landmark || !d_zy_by_landmark))) return SLAM_ERR_INVALID_ARG;
    e->d_obs_zx = d_zx_by_landmark;
    e->d_obs_zy = d_zy_by_landmark;
    e->obs_nlandmarks = nlandmarks;
    e->obs_list_valid = false;
    e->obs_table_owned = false;   // the caller may rewrite the arrays between launches: a list made from them is never reused
    return SLAM_OK;
}

// What every landmark-update stage puts into an EkfArgs alike: the caller's maps, strides, poses and gather index, the engine's
// observation table and its log-likelihood buffer (what slam_logweight_ekf_dev will consume; ll_buf must hold n floats), an
// optional second copy of the log-likelihoods for the caller.  xcd_chunk belongs to the launchers.
static EkfArgs ekf_args(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride, int nlandmarks,
                        const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n, float meas_var,
                        float* d_loglik_user)
{
    EkfArgs a;
    a.map_in = d_map_in;
    a.map_out = d_map_out;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x = d_x;
    a.y = d_y;
    a.th = d_th;
    a.anc = d_anc;
    a.n = n;
    a.obs_zx = e->d_obs_zx;
    a.obs_zy = e->d_obs_zy;
    a.meas_var = meas_var;
    a.loglik = e->ll_buf.as<float>();
    a.loglik_user = d_loglik_user;
    a.xcd_chunk = 0;
    return a;
}

// the split layout's part (SplitIO::map_anc is the caller's business: only the fused front gathers poses and maps differently)
static void apply_split(EkfArgs& a, const SplitIO& s)
{
    a.group_filter = s.group_filter;
    a.cov = s.cov;
    a.cov_stride = s.cov_stride;
    a.covx = s.covx;
    a.covx_stride = s.covx_stride;
    a.cls_in = s.cls_in;
    a.cls_out = s.cls_out;
    a.cstamp = s.cstamp;
    a.stamp_now = s.stamp_now;
}

int slam_ekf_update_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                        int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc,
                        int n, float meas_var, float* d_loglik)
{
    SLAM_ENTER(e);
    if (n < 0 || nlandmarks < 0 || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        !(meas_var > 0.0f) || (n > 0 && (!d_map_in || !d_map_out || !d_x || !d_y || !d_th)))
        return SLAM_ERR_INVALID_ARG;
    if (d_anc && d_map_in == d_map_out) return SLAM_ERR_INVALID_ARG;
    if (e->obs_nlandmarks < 0 || e->obs_nlandmarks != nlandmarks) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    const EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, d_loglik);
    if (d_map_in == d_map_out) {
        // in place: whole rows, or — when the last list that was built had few observations — the observed landmarks only
        const bool can_list = nlandmarks <= kObsListMaxLandmarks;
        if (!e->obs_table_owned) e->obs_list_valid = false;   // the caller's arrays may have been rewritten since the last launch
        const bool sparse = can_list && (e->ekf_inplace_form >= 0 ? e->ekf_inplace_form == 1
                                                                  : e->h_obs[1] == nlandmarks && 4 * (int64_t)e->h_obs[0] <= nlandmarks);
        const bool build = can_list && !e->obs_list_valid && (sparse || e->ekf_inplace_form < 0);
        const size_t L = (size_t)nlandmarks;
        ObsListOut ol;     // where the list is built ...
        ObsListView olv;   // ... and read
        if (build || sparse) {
            if (e->obs_list.cap < 4 * (4 * L + 2)) {
                SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
                SLAM_HIP_TRY(e, e->obs_list.ensure(4 * (4 * L + 2)));
                e->obs_list_valid = false;
            }
            int32_t* li = e->obs_list.as<int32_t>();
            ol = ObsListOut{ li, (float*)(li + L), (float*)(li + 2 * L), li + 3 * L, li + 4 * L };
            olv = ObsListView{ ol.id, ol.zx, ol.zy, ol.round, ol.count };
        }
        auto build_list = [&]() -> hipError_t {
            e->obs_list_valid = true;
            return launch_build_obs_list(e->stream, e->d_obs_zx, e->d_obs_zy, nlandmarks, ol, e->d_hobs);
        };
        if (sparse) {
            if (!e->obs_list_valid) SLAM_HIP_TRY(e, build_list());
            SLAM_HIP_TRY(e, launch_ekf_sparse(e->stream, a, olv, e->prof_next(SLAM_PROF_EKF)));
        } else {
            SLAM_HIP_TRY(e, launch_ekf_update(e->stream, a, e->prof_next(SLAM_PROF_EKF), 0));
            if (build) SLAM_HIP_TRY(e, build_list());   // after the update: only the count for the next frames is wanted
        }
        e->ekf_inplace_launches[sparse ? 1 : 0]++;
    } else {
        const int group = nlandmarks > 128 ? e->ekf_group_size(n, d_anc != nullptr, plane_stride, false) : 0;
        SLAM_HIP_TRY(e, launch_ekf_update(e->stream, a, e->prof_next(SLAM_PROF_EKF), group));
        e->ekf_form_launches[group ? 1 : 0]++;
    }
    e->ll_n = n;
    return SLAM_OK;
}

// meas_cov as the 2x2 stages accept it; leaves the reason behind otherwise
static bool aniso_cov_from(slam_engine* e, const float meas_cov[3], EkfAnisoCov* q)
{
    *q = ekf_aniso_cov(meas_cov);
    if (ekf_aniso_cov_ok(*q)) return true;
    snprintf(e->err, sizeof e->err, "meas_cov must be finite with qxx > 0, qyy > 0 and qxx * qyy - qxy * qxy > 0 in float32");
    return false;
}

int slam_ekf_update_aniso_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                              const float meas_cov[3], float* d_loglik)
{
    SLAM_ENTER(e);
    if (n < 0 || nlandmarks < 0 || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride || !meas_cov ||
        (n > 0 && (!d_map_in || !d_map_out || !d_x || !d_y || !d_th)))
        return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!aniso_cov_from(e, meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (d_anc && d_map_in == d_map_out) return SLAM_ERR_INVALID_ARG;
    if (e->obs_nlandmarks < 0 || e->obs_nlandmarks != nlandmarks) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    // (meas_var of the arguments is not read by this form)
    const EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, 0.0f, d_loglik);
    SLAM_HIP_TRY(e, launch_ekf_aniso(e->stream, a, q, e->prof_next(SLAM_PROF_EKF)));
    e->ekf_aniso_launches++;
    e->ll_n = n;
    return SLAM_OK;
}

int slam_ekf_aniso_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->ekf_aniso_launches;
    return SLAM_OK;
}

/* ------------------------------------------------------------------ data association (assoc_kernels.hip) */

int slam_detections_upload_host(slam_engine* e, const float* zx, const float* zy, int ndet)
{
    SLAM_ENTER(e);
    if (ndet < 0 || ndet > SLAM_MAX_DETECTIONS || (ndet > 0 && (!zx || !zy))) return SLAM_ERR_INVALID_ARG;
    const float big = std::numeric_limits<float>::max();
    for (int k = 0; k < ndet; ++k)
        if (!(zx[k] >= -big && zx[k] <= big && zy[k] >= -big && zy[k] <= big)) return SLAM_ERR_INVALID_ARG;   // (NaN fails every comparison)
    if (!e->det_buf.p) SLAM_HIP_TRY(e, e->det_buf.ensure(sizeof(float) * 2 * SLAM_MAX_DETECTIONS));
    if (ndet > 0) {
        float* h = e->stage_acquire();
        for (int k = 0; k < SLAM_MAX_DETECTIONS; ++k) {   // zx[64] | zy[ndet]: one copy
            h[k] = k < ndet ? zx[k] : 0.0f;
            if (k < ndet) h[SLAM_MAX_DETECTIONS + k] = zy[k];
        }
        const hipError_t err = hipMemcpyAsync(e->det_buf.as<float>(), h, sizeof(float) * (SLAM_MAX_DETECTIONS + (size_t)ndet),
                                              hipMemcpyHostToDevice, e->stream);
        SLAM_HIP_TRY(e, e->stage_release(h));
        SLAM_HIP_TRY(e, err);
    }
    e->d_det_zx = e->det_buf.as<float>();
    e->d_det_zy = e->det_buf.as<float>() + SLAM_MAX_DETECTIONS;
    e->ndet = ndet;
    e->det_pending = false;   // (a detector launch still in flight wrote the buffer in front of this copy, in stream order)
    e->det_from_scan = false;
    return SLAM_OK;
}

int slam_detections_set_dev(slam_engine* e, const float* d_zx, const float* d_zy, int ndet)
{
    SLAM_ENTER(e);
    if (ndet < 0 || ndet > SLAM_MAX_DETECTIONS || (ndet > 0 && (!d_zx || !d_zy))) return SLAM_ERR_INVALID_ARG;
    e->d_det_zx = d_zx;
    e->d_det_zy = d_zy;
    e->ndet = ndet;
    e->det_pending = false;
    e->det_from_scan = false;
    return SLAM_OK;
}

// the argument checks the two associating stages share (everything but the measurement noise)
static bool associate_args_ok(const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                              const float* d_th, int n, float gate, float new_gate, int create, const uint8_t* d_assoc, int assoc_stride)
{
    return !(n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
             assoc_stride < nlandmarks || !(gate > 0.0f && gate <= std::numeric_limits<float>::max()) || !(new_gate >= gate) ||
             (create != 0 && create != 1) || (n > 0 && (!d_map || !d_x || !d_y || !d_th || !d_assoc)));
}

// ... and what they put into an AssocArgs alike: the caller's rows, poses, gather index and table, the engine's detections
static AssocArgs assoc_args(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                            const float* d_y, const float* d_th, const int32_t* d_anc, int n, float meas_var, float gate, float new_gate,
                            uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    AssocArgs a;
    a.map = d_map;
    a.row_stride = row_stride;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x = d_x;
    a.y = d_y;
    a.th = d_th;
    a.anc = d_anc;
    a.n = n;
    a.det_zx = e->d_det_zx;
    a.det_zy = e->d_det_zy;
    a.ndet = e->ndet;
    a.meas_var = meas_var;
    a.gate = gate;
    a.new_gate = new_gate;
    a.assoc = d_assoc;
    a.assoc_stride = assoc_stride;
    a.stats = d_stats;
    a.xcd_chunk = 0;
    return a;
}

int slam_associate_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                       const float* d_y, const float* d_th, const int32_t* d_anc, int n, float meas_var, float gate, float new_gate,
                       int create, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (!associate_args_ok(d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, new_gate, create, d_assoc, assoc_stride) ||
        !(meas_var > 0.0f))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    const AssocArgs a = assoc_args(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, gate, new_gate,
                                   d_assoc, assoc_stride, d_stats);
    SLAM_HIP_TRY(e, launch_associate(e->stream, a, create != 0, e->prof_next(SLAM_PROF_PAGES)));
    e->assoc_launches[0]++;
    return SLAM_OK;
}

int slam_associate_aniso_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                             const float* d_y, const float* d_th, const int32_t* d_anc, int n, const float meas_cov[3], float gate,
                             float new_gate, int create, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (!associate_args_ok(d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, new_gate, create, d_assoc, assoc_stride) ||
        !meas_cov)
        return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!aniso_cov_from(e, meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    // (meas_var of the arguments is not read by this form)
    const AssocArgs a = assoc_args(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, 0.0f, gate, new_gate, d_assoc,
                                   assoc_stride, d_stats);
    SLAM_HIP_TRY(e, launch_associate_aniso(e->stream, a, q, create != 0, e->prof_next(SLAM_PROF_PAGES)));
    e->assoc_aniso_launches[0]++;
    return SLAM_OK;
}

int slam_ekf_update_assoc_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                              float meas_var, const uint8_t* d_assoc, int assoc_stride, float* d_loglik)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || !(meas_var > 0.0f) || (n > 0 && (!d_map_in || !d_map_out || !d_x || !d_y || !d_th || !d_assoc)))
        return SLAM_ERR_INVALID_ARG;
    if (d_anc && d_map_in == d_map_out) return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    // (the observation table of the arguments is not read by this form)
    const EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, d_loglik);
    const EkfAssocTable tab{ d_assoc, assoc_stride, e->d_det_zx, e->d_det_zy, e->ndet };
    SLAM_HIP_TRY(e, launch_ekf_assoc(e->stream, a, tab, e->prof_next(SLAM_PROF_EKF)));
    e->assoc_launches[1]++;
    e->ll_n = n;
    return SLAM_OK;
}

int slam_ekf_update_assoc_aniso_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                                    int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                    const float meas_cov[3], const uint8_t* d_assoc, int assoc_stride, float* d_loglik)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || !meas_cov || (n > 0 && (!d_map_in || !d_map_out || !d_x || !d_y || !d_th || !d_assoc)))
        return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!aniso_cov_from(e, meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (d_anc && d_map_in == d_map_out) return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    // (neither the observation table nor meas_var of the arguments is read by this form)
    const EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, 0.0f, d_loglik);
    const EkfAssocTable tab{ d_assoc, assoc_stride, e->d_det_zx, e->d_det_zy, e->ndet };
    SLAM_HIP_TRY(e, launch_ekf_assoc_aniso(e->stream, a, tab, q, e->prof_next(SLAM_PROF_EKF)));
    e->assoc_aniso_launches[1]++;
    e->ll_n = n;
    return SLAM_OK;
}

int slam_assoc_aniso_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->assoc_aniso_launches[0];
    counts[1] = e->assoc_aniso_launches[1];
    return SLAM_OK;
}

int slam_assoc_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->assoc_launches[0];
    counts[1] = e->assoc_launches[1];
    return SLAM_OK;
}

/* ------------------------------------------------------------------ the detector (detect_kernels.hip) */

void slam_detect_params_default(slam_detect_params* p)
{
    if (!p) return;
    p->jump = 0.3f;
    p->guard = 1.0f;
    p->max_width = 0.5f;
    p->max_range = 20.0f;
    p->min_points = 3;
    p->max_points = 40;
    p->wrap = 1;
}

int slam_detect_scan_dev(slam_engine* e, const slam_detect_params* params, int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (!params) return SLAM_ERR_INVALID_ARG;
    if (!slam_detect_params_ok(params)) {
        snprintf(e->err, sizeof e->err, "the detector needs finite jump, guard, max_width and max_range > 0, guard >= jump, "
                                        "1 <= min_points <= max_points <= %d and wrap in {0, 1}", (int)SLAM_DETECT_MAX_POINTS);
        return SLAM_ERR_INVALID_ARG;
    }
    if (e->nbeams < 0) return SLAM_ERR_NOT_READY;
    if (!e->det_buf.p) SLAM_HIP_TRY(e, e->det_buf.ensure(sizeof(float) * 2 * SLAM_MAX_DETECTIONS));
    DetectArgs a;
    a.bx = e->d_bx;
    a.by = e->d_by;
    a.nbeams = e->nbeams;
    a.jump2 = params->jump * params->jump;   // one float32 product each (-ffp-contract=off)
    a.guard2 = params->guard * params->guard;
    a.width2 = params->max_width * params->max_width;
    a.range2 = params->max_range * params->max_range;
    a.min_points = params->min_points;
    a.max_points = params->max_points;
    a.wrap = params->wrap;
    a.det = e->det_buf.as<float>();
    a.stats = d_stats;
    a.h_out = e->d_hdet;
    a.seq = e->det_seq + 1;
    SLAM_HIP_TRY(e, launch_detect_scan(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->det_seq = a.seq;
    e->d_det_zx = e->det_buf.as<float>();
    e->d_det_zy = e->det_buf.as<float>() + SLAM_MAX_DETECTIONS;
    e->ndet = 0;   // until the count is picked up
    e->det_pending = true;
    e->det_from_scan = true;
    e->detect_launches++;
    return SLAM_OK;
}

int slam_detect_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->detect_launches;
    return SLAM_OK;
}

int slam_detections_get_host(slam_engine* e, float* zx, float* zy, int32_t* ndet)
{
    SLAM_ENTER(e);
    if (!zx || !zy || !ndet) return SLAM_ERR_INVALID_ARG;
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    // the detector's output: the whole block as its kernel left it (0 from ndet on); anything else: ndet values, 0 behind them
    const size_t count = e->det_from_scan ? (size_t)SLAM_MAX_DETECTIONS : (size_t)e->ndet;
    for (size_t k = count; k < SLAM_MAX_DETECTIONS; ++k) zx[k] = zy[k] = 0.0f;
    if (count > 0) {
        SLAM_HIP_TRY(e, hipMemcpyAsync(zx, e->d_det_zx, sizeof(float) * count, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipMemcpyAsync(zy, e->d_det_zy, sizeof(float) * count, hipMemcpyDeviceToHost, e->stream));
    }
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    *ndet = e->ndet;
    return SLAM_OK;
}

/* ------------------------------------------------------------------ landmark existence evidence (evidence_kernels.hip) */

int slam_landmark_evidence_dev(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                               const float* d_y, const int32_t* d_anc, int n, const uint8_t* d_assoc, int assoc_stride,
                               const uint8_t* d_ev_in, uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax, float view_range,
                               int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
        assoc_stride < nlandmarks || ev_stride < nlandmarks || hit < 1 || hit > 255 || miss < 1 || miss > 255 || cmax < 1 || cmax > 255 ||
        !(view_range > 0.0f && view_range <= std::numeric_limits<float>::max()) ||   // (NaN fails every comparison)
        !d_map || !d_x || !d_y || !d_assoc || !d_ev_in || !d_ev_out || (d_anc && d_ev_in == d_ev_out))
        return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
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
    a.xcd_chunk = 0;
    SLAM_HIP_TRY(e, launch_landmark_evidence(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->evidence_launches[0]++;
    return SLAM_OK;
}

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

int slam_evidence_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->evidence_launches[0];
    counts[1] = e->evidence_launches[1];
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

int slam_frame_front_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                         const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id, const float dp[3],
                         const float sigma[3], uint64_t seed, uint32_t frame, float* d_score, int32_t* d_count,
                         const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride, int nlandmarks,
                         float meas_var, bool* launched, const slam::SplitIO* split, float* d_obs_save)
{
    SLAM_ENTER(e);
    *launched = false;
    if (!e->frame_fusion) return SLAM_OK;
    if (e->prof_mask & (1 << SLAM_PROF_SCORE)) return SLAM_OK;   // the score stage is being timed: it stays a launch of its own
    // the checks of slam_motion_score_dev and of slam_ekf_update_dev (out of place)
    if (n <= 0 || first_id < 0 || !dp || !sigma || !d_src_x || !d_src_y || !d_src_th || !d_x || !d_y || !d_th || !d_score ||
        !d_count || !d_anc || !d_map_in || !d_map_out || d_map_in == d_map_out)
        return SLAM_OK;   // the two calls will say what is wrong
    if (d_src_x == d_x || d_src_y == d_y || d_src_th == d_th) return SLAM_ERR_INVALID_ARG;
    if (nlandmarks <= 128 || plane_stride < nlandmarks || row_stride < (split ? 2 : 5) * (int64_t)plane_stride || !(meas_var > 0.0f))
        return SLAM_OK;
    if (int rc = check_score_inputs(e, slot)) return rc;
    if (e->obs_nlandmarks < 0 || e->obs_nlandmarks != nlandmarks) return SLAM_ERR_NOT_READY;
    if (d_obs_save && !split) return SLAM_ERR_INVALID_ARG;
    const int group = e->ekf_group_size(n, true, plane_stride, true, split != nullptr);
    if (!frame_front_fits(n, nlandmarks, group)) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    // (a.x / a.y / a.th are not read by the fused launch: the update works out its motion samples itself)
    EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th,
                         split && split->map_anc ? split->map_anc : d_anc, n, meas_var, nullptr);
    if (split) apply_split(a, *split);
    MotionIO io{ d_src_x, d_src_y, d_src_th, d_anc, d_x, d_y, d_th, FreeListRider() };
    int lanes = 0;
    // one bracket for the whole launch: it counts as the frame's landmark update (the dominant stage)
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, n, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_frame_front(e->stream, sg, e->d_bx, e->d_by, e->nbeams, io, first_id, dp, sigma, seed,
                                       frame, d_score, d_count, a, group, e->prof_next(SLAM_PROF_EKF), launched, &lanes, d_obs_save));
    if (*launched) {
        e->front_last[0] = group;
        e->front_last[1] = lanes;
        e->ll_n = n;
        e->ekf_form_launches[1]++;
        e->front_launches++;
    }
    return SLAM_OK;
}

int slam_ekf_split_dev(slam_engine* e, const float* d_mean_in, float* d_mean_out, int64_t row_stride, int plane_stride,
                       int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                       float meas_var, const slam::SplitIO* split)
{
    SLAM_ENTER(e);
    if (n <= 0 || nlandmarks <= 0 || plane_stride < nlandmarks || row_stride < 2 * (int64_t)plane_stride || !(meas_var > 0.0f) ||
        !d_mean_in || !d_mean_out || d_mean_in == d_mean_out || !d_x || !d_y || !d_th || !split || !split->cov || !split->covx || !split->cls_in ||
        !split->cls_out || !split->cstamp)
        return SLAM_ERR_INVALID_ARG;
    if (e->obs_nlandmarks < 0 || e->obs_nlandmarks != nlandmarks) return SLAM_ERR_NOT_READY;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    EkfArgs a = ekf_args(e, d_mean_in, d_mean_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, nullptr);
    apply_split(a, *split);
    // the tail of a sharded fused frame (group_filter 2) must group the particles as the front launch did
    const int group = split->group_filter == 2 ? e->front_last[0] : e->ekf_group_size(n, d_anc != nullptr, plane_stride, false, true);
    SLAM_HIP_TRY(e, launch_ekf_update(e->stream, a, e->prof_next(split->group_filter == 2 ? SLAM_PROF_EKF_TAIL : SLAM_PROF_EKF), group));
    if (split->group_filter != 2) e->ekf_form_launches[1]++;
    e->ll_n = n;
    return SLAM_OK;
}

int slam_ekf_materialise_dev(slam_engine* e, const float* d_mean_in, float* d_mean_out, int64_t row_stride, int plane_stride,
                             int nlandmarks, const float* d_obs_save, const float* d_x, const float* d_y, const float* d_th,
                             const int32_t* d_anc, int n, float meas_var, const slam::SplitIO* split, const uint32_t* d_survivor,
                             uint32_t stamp, int group)
{
    SLAM_ENTER(e);
    if (n <= 0 || nlandmarks <= 0 || plane_stride < nlandmarks || row_stride < 2 * (int64_t)plane_stride || !(meas_var > 0.0f) ||
        !d_mean_in || !d_mean_out || d_mean_in == d_mean_out || !d_obs_save || !d_x || !d_y || !d_th || !split || !split->cov ||
        !split->covx || !split->cls_in)
        return SLAM_ERR_INVALID_ARG;
    EkfArgs a = ekf_args(e, d_mean_in, d_mean_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, meas_var, nullptr);
    apply_split(a, *split);
    a.obs_zx = d_obs_save;   // the table as the frame's own update saw it
    a.obs_zy = d_obs_save + plane_stride;
    a.loglik = nullptr;      // (nothing but mean rows is written)
    a.cls_out = nullptr;
    a.cstamp = nullptr;
    a.group_filter = 0;
    a.survivor = d_survivor;
    a.survivor_stamp = stamp;
    SLAM_HIP_TRY(e, launch_ekf_materialise(e->stream, a, e->prof_next(SLAM_PROF_MATERIALISE), group));
    return SLAM_OK;
}

int slam_survivor_rows_set(slam_engine* e, int on)
{
    SLAM_ENTER(e);
    if (on < 0 || on > 1) return SLAM_ERR_INVALID_ARG;
    e->survivor_rows = on != 0;
    return SLAM_OK;
}

int slam_frame_fusion_set(slam_engine* e, int on)
{
    SLAM_ENTER(e);
    if (on < 0 || on > 1) return SLAM_ERR_INVALID_ARG;
    e->frame_fusion = on != 0;
    return SLAM_OK;
}

int slam_frame_fusion_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->front_launches;
    return SLAM_OK;
}

int slam_frame_front_last(slam_engine* e, int32_t info[2])
{
    SLAM_ENTER(e);
    if (!info) return SLAM_ERR_INVALID_ARG;
    info[0] = e->front_last[0];
    info[1] = e->front_last[1];
    return SLAM_OK;
}

int slam_ekf_form_set(slam_engine* e, int form)
{
    SLAM_ENTER(e);
    if (form < -1 || form > 2) return SLAM_ERR_INVALID_ARG;
    e->ekf_form = form;
    return SLAM_OK;
}

int slam_pf_paged_set(slam_engine* e, int on)
{
    SLAM_ENTER(e);
    if (on < 0 || on > 1) return SLAM_ERR_INVALID_ARG;
    e->pf_paged = on != 0;
    return SLAM_OK;
}

int slam_ekf_inplace_form_set(slam_engine* e, int form)
{
    SLAM_ENTER(e);
    if (form < -1 || form > 1) return SLAM_ERR_INVALID_ARG;
    e->ekf_inplace_form = form;
    return SLAM_OK;
}

int slam_ekf_inplace_form_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->ekf_inplace_launches[0];
    counts[1] = e->ekf_inplace_launches[1];
    return SLAM_OK;
}

int slam_ekf_form_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->ekf_form_launches[0];
    counts[1] = e->ekf_form_launches[1];
    return SLAM_OK;
}

}  // extern "C"
