// engine_assoc.hip — what a frame of detections without identity adds behind the C ABI: the detections themselves (uploaded, set,
// or made from the scan by the detector; optionally a covariance per detection), the association stage with meas_var * I, a 2x2 Q
// or the detections' own Q_k, and the weight of what it leaves unexplained.  The landmark update under the table the association
// makes: engine_ekf.hip; the landmarks' existence evidence: engine_evidence.hip.

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
    e->det_has_cov = false;
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
    e->det_has_cov = false;
    return SLAM_OK;
}

int slam_detections_cov_upload_host(slam_engine* e, const float* qxx, const float* qxy, const float* qyy, int ndet)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (ndet != e->ndet || (ndet > 0 && (!qxx || !qxy || !qyy))) return SLAM_ERR_INVALID_ARG;
    for (int k = 0; k < ndet; ++k) {
        const float q3[3] = { qxx[k], qxy[k], qyy[k] };
        EkfAnisoCov q;
        if (!slam_aniso_cov_from(e, q3, &q)) return SLAM_ERR_INVALID_ARG;
    }
    if (!e->detcov_buf.p) SLAM_HIP_TRY(e, e->detcov_buf.ensure(sizeof(float) * 3 * SLAM_MAX_DETECTIONS));
    if (ndet > 0) {
        float* h = e->stage_acquire();
        for (int k = 0; k < SLAM_MAX_DETECTIONS; ++k) {   // qxx[64] | qxy[64] | qyy[64], the identity from ndet on: one copy
            h[k] = k < ndet ? qxx[k] : 1.0f;
            h[SLAM_MAX_DETECTIONS + k] = k < ndet ? qxy[k] : 0.0f;
            h[2 * SLAM_MAX_DETECTIONS + k] = k < ndet ? qyy[k] : 1.0f;
        }
        const hipError_t err = hipMemcpyAsync(e->detcov_buf.as<float>(), h, sizeof(float) * 3 * SLAM_MAX_DETECTIONS, hipMemcpyHostToDevice, e->stream);
        SLAM_HIP_TRY(e, e->stage_release(h));
        SLAM_HIP_TRY(e, err);
    }
    // (ndet == 0: nothing was copied and nothing reads the three arrays; they point into the buffer all the same)
    e->d_det_qxx = e->detcov_buf.as<float>();
    e->d_det_qxy = e->detcov_buf.as<float>() + SLAM_MAX_DETECTIONS;
    e->d_det_qyy = e->detcov_buf.as<float>() + 2 * SLAM_MAX_DETECTIONS;
    e->det_has_cov = true;
    return SLAM_OK;
}

int slam_detections_cov_set_dev(slam_engine* e, const float* d_qxx, const float* d_qxy, const float* d_qyy, int ndet)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    if (ndet != e->ndet || (ndet > 0 && (!d_qxx || !d_qxy || !d_qyy))) return SLAM_ERR_INVALID_ARG;
    e->d_det_qxx = d_qxx;
    e->d_det_qxy = d_qxy;
    e->d_det_qyy = d_qyy;
    e->det_has_cov = true;
    return SLAM_OK;
}

int slam_detections_get_cov_host(slam_engine* e, float* qxx, float* qxy, float* qyy, int32_t* ndet)
{
    SLAM_ENTER(e);
    if (!qxx || !qxy || !qyy || !ndet) return SLAM_ERR_INVALID_ARG;
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (e->ndet < 0 || !e->det_has_cov) return SLAM_ERR_NOT_READY;
    const size_t count = (size_t)e->ndet;
    if (count > 0) {
        SLAM_HIP_TRY(e, hipMemcpyAsync(qxx, e->d_det_qxx, sizeof(float) * count, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipMemcpyAsync(qxy, e->d_det_qxy, sizeof(float) * count, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipMemcpyAsync(qyy, e->d_det_qyy, sizeof(float) * count, hipMemcpyDeviceToHost, e->stream));
    }
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    *ndet = e->ndet;
    return SLAM_OK;
}

// the argument checks of the association stage (everything but the measurement noise)
static bool associate_args_ok(const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x, const float* d_y,
                              const float* d_th, int n, float gate, float new_gate, int create, const uint8_t* d_assoc, int assoc_stride)
{
    return !(n < 0 || nlandmarks < 0 || nlandmarks > SLAM_MAX_OBS || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride ||
             assoc_stride < nlandmarks || !(gate > 0.0f && gate <= std::numeric_limits<float>::max()) || !(new_gate >= gate) ||
             (create != 0 && create != 1) || (n > 0 && (!d_map || !d_x || !d_y || !d_th || !d_assoc)));
}

// ... and what it puts into an AssocArgs: the caller's rows, poses, gather index and table, the engine's detections
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

int slam_engine_associate(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                          const float* d_y, const float* d_th, const int32_t* d_anc, int n, const slam_meas_noise& noise, float gate,
                          float new_gate, int create, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (!associate_args_ok(d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, n, gate, new_gate, create, d_assoc, assoc_stride) ||
        (noise.per_det ? false : noise.full ? !noise.meas_cov : !(noise.meas_var > 0.0f)))
        return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!noise.per_det && noise.full && !slam_aniso_cov_from(e, noise.meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (e->ndet < 0 || (noise.per_det && !e->det_has_cov)) return SLAM_ERR_NOT_READY;
    if (n == 0) return SLAM_OK;
    // (meas_var of the arguments is not read under a covariance)
    const AssocArgs a = assoc_args(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n,
                                   noise.per_det || noise.full ? 0.0f : noise.meas_var, gate, new_gate, d_assoc, assoc_stride, d_stats);
    const DetCovArgs dq{ e->d_det_qxx, e->d_det_qxy, e->d_det_qyy, e->ndet };
    SLAM_HIP_TRY(e, launch_associate(e->stream, a, !noise.per_det && noise.full ? &q : nullptr, noise.per_det ? &dq : nullptr, create != 0,
                                     e->prof_next(SLAM_PROF_PAGES)));
    (noise.per_det ? e->assoc_detcov_launches : noise.full ? e->assoc_aniso_launches : e->assoc_launches)[0]++;
    return SLAM_OK;
}

int slam_associate_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                       const float* d_y, const float* d_th, const int32_t* d_anc, int n, float meas_var, float gate, float new_gate,
                       int create, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    return slam_engine_associate(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, slam_meas_noise{ meas_var, nullptr, false },
                                 gate, new_gate, create, d_assoc, assoc_stride, d_stats);
}

int slam_associate_aniso_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                             const float* d_y, const float* d_th, const int32_t* d_anc, int n, const float meas_cov[3], float gate,
                             float new_gate, int create, uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    return slam_engine_associate(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, slam_meas_noise{ 0.0f, meas_cov, true },
                                 gate, new_gate, create, d_assoc, assoc_stride, d_stats);
}

int slam_associate_detcov_dev(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks, const float* d_x,
                              const float* d_y, const float* d_th, const int32_t* d_anc, int n, float gate, float new_gate, int create,
                              uint8_t* d_assoc, int assoc_stride, int32_t* d_stats)
{
    return slam_engine_associate(e, d_map, row_stride, plane_stride, nlandmarks, d_x, d_y, d_th, d_anc, n, slam_meas_noise{ 0.0f, nullptr, false, true },
                                 gate, new_gate, create, d_assoc, assoc_stride, d_stats);
}

int slam_assoc_detcov_counts(slam_engine* e, int64_t counts[2])
{
    SLAM_ENTER(e);
    if (!counts) return SLAM_ERR_INVALID_ARG;
    counts[0] = e->assoc_detcov_launches[0];
    counts[1] = e->assoc_detcov_launches[1];
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

void slam_detect_fit_default(slam_detect_fit* f)
{
    if (!f) return;
    f->radius = 0.1f;
    f->spread_tol = 0.0f;
}

// the one checked path of the three entry points (fit == nullptr: the centroid, the kernel instantiation without the fit;
// noise == nullptr: the instantiations without the noise model — the detections then carry no covariance)
static int detect_scan(slam_engine* e, const slam_detect_params* params, const slam_detect_fit* fit, const slam_detect_noise* noise,
                       int32_t* d_stats)
{
    SLAM_ENTER(e);
    if (!params) return SLAM_ERR_INVALID_ARG;
    if (!slam_detect_params_ok(params)) {
        slam_detect_params_error(e);
        return SLAM_ERR_INVALID_ARG;
    }
    if (fit && !slam_detect_fit_ok(fit)) {
        slam_detect_fit_error(e);
        return SLAM_ERR_INVALID_ARG;
    }
    if (noise && !slam_detect_noise_ok(noise)) {
        slam_detect_noise_error(e);
        return SLAM_ERR_INVALID_ARG;
    }
    if (e->nbeams < 0) return SLAM_ERR_NOT_READY;
    if (!e->det_buf.p) SLAM_HIP_TRY(e, e->det_buf.ensure(sizeof(float) * 2 * SLAM_MAX_DETECTIONS));
    if (noise && !e->detcov_buf.p) SLAM_HIP_TRY(e, e->detcov_buf.ensure(sizeof(float) * 3 * SLAM_MAX_DETECTIONS));
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
    a.fit = fit ? 1 : 0;
    a.rho2 = fit ? fit->radius * fit->radius : 0.0f;
    a.lim = fit ? a.rho2 + fit->spread_tol * fit->spread_tol : 0.0f;
    const DetectNoiseArgs nz{ noise ? noise->range_var : 0.0f, noise ? noise->bearing_var : 0.0f, noise ? noise->lateral_var : 0.0f,
                              noise ? e->detcov_buf.as<float>() : nullptr };
    SLAM_HIP_TRY(e, launch_detect_scan(e->stream, a, e->prof_next(SLAM_PROF_PAGES), noise ? &nz : nullptr));
    e->det_seq = a.seq;
    e->d_det_zx = e->det_buf.as<float>();
    e->d_det_zy = e->det_buf.as<float>() + SLAM_MAX_DETECTIONS;
    e->ndet = 0;   // until the count is picked up
    e->det_pending = true;
    e->det_from_scan = true;
    e->det_has_cov = noise != nullptr;   // the model's Q_k beside the detections, in the engine's own buffer
    if (noise) {
        e->d_det_qxx = e->detcov_buf.as<float>();
        e->d_det_qxy = e->detcov_buf.as<float>() + SLAM_MAX_DETECTIONS;
        e->d_det_qyy = e->detcov_buf.as<float>() + 2 * SLAM_MAX_DETECTIONS;
        e->detect_noise_launches++;
    }
    e->detect_launches++;
    if (fit) e->detect_fit_launches++;
    return SLAM_OK;
}

int slam_detect_scan_dev(slam_engine* e, const slam_detect_params* params, int32_t* d_stats)
{
    return detect_scan(e, params, nullptr, nullptr, d_stats);
}

int slam_detect_scan_fit_dev(slam_engine* e, const slam_detect_params* params, const slam_detect_fit* fit, int32_t* d_stats)
{
    return detect_scan(e, params, fit, nullptr, d_stats);
}

int slam_detect_scan_noise_dev(slam_engine* e, const slam_detect_params* params, const slam_detect_fit* fit, const slam_detect_noise* noise,
                               int32_t* d_stats)
{
    return detect_scan(e, params, fit, noise, d_stats);
}

int slam_detect_noise_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->detect_noise_launches;
    return SLAM_OK;
}

int slam_detect_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->detect_launches;
    return SLAM_OK;
}

int slam_detect_fit_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->detect_fit_launches;
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

/* ------------------------------------------------------------------ what the association leaves unexplained (assoc_weight_kernels.hip) */

int slam_assoc_weight_dev(slam_engine* e, const int32_t* d_stats, const int32_t* d_missed, int n, float log_new, float log_clutter,
                          float log_miss, float* d_loglik, float* d_terms)
{
    SLAM_ENTER(e);
    if (n < 0 || !d_stats || !assoc_weight_const_ok(log_new) || !assoc_weight_const_ok(log_clutter) || !assoc_weight_const_ok(log_miss))
        return SLAM_ERR_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    if (!d_loglik && e->ll_n != n) return SLAM_ERR_NOT_READY;   // needs the landmark update of n particles on this engine first
    const AssocWeightArgs a{ d_stats, d_missed, n, log_new, log_clutter, log_miss, d_loglik ? d_loglik : e->ll_buf.as<float>(), d_terms };
    SLAM_HIP_TRY(e, launch_assoc_weight(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->assoc_weight_launches++;
    return SLAM_OK;
}

int slam_assoc_weight_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->assoc_weight_launches;
    return SLAM_OK;
}

}  // extern "C"
