// engine_ekf.hip — the landmark side of a particle-filter frame behind the C ABI: motion sample (alone, or with the score of
// the sampled poses), the observation table, the landmark update in every form (in place, out of place, split layout, fused
// with motion + score as the frame's front launch; on rows with meas_var * I or a 2x2 Q, from the frame's table or through a
// per-particle association table) and the switches and counters of those forms.  Detections, association, evidence: engine_assoc.hip.

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <limits>

#include "engine_internal.h"

using namespace slam;

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

// the isotropic update from the frame's table alone has more than one kernel per direction: in place whole rows or the observed
// landmarks only, out of place one wavefront per particle or grouped
static int launch_iso_frame_update(slam_engine* e, const EkfArgs& a)
{
    const int nlandmarks = a.nlandmarks;
    if (a.map_in == a.map_out) {
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
        const int group = nlandmarks > 128 ? e->ekf_group_size(a.n, a.anc != nullptr, a.plane_stride, false) : 0;
        SLAM_HIP_TRY(e, launch_ekf_update(e->stream, a, e->prof_next(SLAM_PROF_EKF), group));
        e->ekf_form_launches[group ? 1 : 0]++;
    }
    return SLAM_OK;
}

int slam_engine_ekf_update(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride, int nlandmarks,
                           const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n, const slam_meas_noise& noise,
                           const slam_assoc_view* table, float* d_loglik)
{
    SLAM_ENTER(e);
    if (table)
        if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (n < 0 || nlandmarks < 0 || (table && (nlandmarks > SLAM_MAX_OBS || table->assoc_stride < nlandmarks)) || plane_stride < nlandmarks ||
        row_stride < 5 * (int64_t)plane_stride || (noise.per_det ? !table : noise.full ? !noise.meas_cov : !(noise.meas_var > 0.0f)) ||
        (n > 0 && (!d_map_in || !d_map_out || !d_x || !d_y || !d_th || (table && !table->d_assoc))))
        return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!noise.per_det && noise.full && !slam_aniso_cov_from(e, noise.meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (d_anc && d_map_in == d_map_out) return SLAM_ERR_INVALID_ARG;
    if (table ? e->ndet < 0 : (e->obs_nlandmarks < 0 || e->obs_nlandmarks != nlandmarks)) return SLAM_ERR_NOT_READY;
    if (noise.per_det && !e->det_has_cov) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
    // (under a 2x2 covariance meas_var of the arguments is not read, under a table their observation table is not)
    const EkfArgs a = ekf_args(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                               noise.full || noise.per_det ? 0.0f : noise.meas_var, d_loglik);
    if (noise.per_det) {
        const EkfAssocTable tab{ table->d_assoc, table->assoc_stride, e->d_det_zx, e->d_det_zy, e->ndet };
        const DetCovArgs dq{ e->d_det_qxx, e->d_det_qxy, e->d_det_qyy, e->ndet };
        SLAM_HIP_TRY(e, launch_ekf_rows_detcov(e->stream, a, dq, tab, e->prof_next(SLAM_PROF_EKF)));
        e->assoc_detcov_launches[1]++;
    } else if (!noise.full && !table) {
        if (int rc = launch_iso_frame_update(e, a)) return rc;
    } else {
        const EkfAssocTable tab{ table ? table->d_assoc : nullptr, table ? table->assoc_stride : 0, e->d_det_zx, e->d_det_zy, e->ndet };
        SLAM_HIP_TRY(e, launch_ekf_rows(e->stream, a, noise.full ? &q : nullptr, table ? &tab : nullptr, e->prof_next(SLAM_PROF_EKF)));
        // each form counts in its own counter and in no other
        (!table ? e->ekf_aniso_launches : noise.full ? e->assoc_aniso_launches[1] : e->assoc_launches[1])++;
    }
    e->ll_n = n;
    return SLAM_OK;
}

int slam_ekf_update_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                        int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc,
                        int n, float meas_var, float* d_loglik)
{
    return slam_engine_ekf_update(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                  slam_meas_noise{ meas_var, nullptr, false }, nullptr, d_loglik);
}

int slam_ekf_update_aniso_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                              const float meas_cov[3], float* d_loglik)
{
    return slam_engine_ekf_update(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                  slam_meas_noise{ 0.0f, meas_cov, true }, nullptr, d_loglik);
}

int slam_ekf_update_assoc_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                              float meas_var, const uint8_t* d_assoc, int assoc_stride, float* d_loglik)
{
    const slam_assoc_view table{ d_assoc, assoc_stride };
    return slam_engine_ekf_update(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                  slam_meas_noise{ meas_var, nullptr, false }, &table, d_loglik);
}

int slam_ekf_update_assoc_aniso_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                                    int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                    const float meas_cov[3], const uint8_t* d_assoc, int assoc_stride, float* d_loglik)
{
    const slam_assoc_view table{ d_assoc, assoc_stride };
    return slam_engine_ekf_update(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                  slam_meas_noise{ 0.0f, meas_cov, true }, &table, d_loglik);
}

int slam_ekf_update_assoc_detcov_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                                     int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                     const uint8_t* d_assoc, int assoc_stride, float* d_loglik)
{
    const slam_assoc_view table{ d_assoc, assoc_stride };
    return slam_engine_ekf_update(e, d_map_in, d_map_out, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                  slam_meas_noise{ 0.0f, nullptr, false, true }, &table, d_loglik);
}

int slam_ekf_aniso_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->ekf_aniso_launches;
    return SLAM_OK;
}

int slam_frame_front_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                         const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id, const float dp[3],
                         const float sigma[3], uint64_t seed, uint32_t frame, float* d_score, int32_t* d_count,
                         const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride, int nlandmarks,
                         float meas_var, bool* launched, const slam::SplitIO* split, float* d_obs_save, const slam_front_weights* weights)
{
    SLAM_ENTER(e);
    *launched = false;
    if (weights) *weights->made = false;
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
    // the weights too where one workgroup scores and updates the same particles (no resample gate: its carried weights and its
    // scan stay with the weights' launch); the block maxima go where slam_logweight_dev leaves them
    FrontWeights fw{};
    bool weighted = false;
    if (weights && weights->d_logw && e->gate_frac_q16 == 0) {
        if (int rc = slam_engine_bmax_ready(e)) return rc;
        fw = FrontWeights{ weights->score_gain, weights->d_logw, e->bmax_buf.as<float>(), nullptr, nullptr, &weighted };
    }
    SLAM_HIP_TRY(e, launch_frame_front(e->stream, sg, e->d_bx, e->d_by, e->nbeams, io, first_id, dp, sigma, seed,
                                       frame, d_score, d_count, a, group, e->prof_next(SLAM_PROF_EKF), launched, &lanes, d_obs_save,
                                       fw.logw ? &fw : nullptr));
    if (weighted) {
        e->bmax_count = (n + 63) / 64;
        e->bmax_n = n;
        *weights->made = true;
    }
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
