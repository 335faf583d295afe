// pf_session.hip — the session object of the slam_pf_* interface (pf_session.h): made and destroyed, reset and loaded (poses, maps),
// its option switches (refinement, 2x2 measurement covariance, association, pruning, the detector, a known map) and its small counters.
// The storage forms are pf_session_store.hip, the frame pf_session_frame.hip, the read-backs pf_session_read.hip.

#include <float.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <new>
#include <vector>

#include "pf_session.h"

namespace slam::session {
namespace {

// Pruning: the evidence of the current maps, from scratch — a map that is there is trusted (seen: cmax, else 0).  At the switch,
// and whenever the session's maps are replaced wholesale while pruning is on.
int evidence_from_maps(slam_pf* pf)
{
    if (!pf->prune_on) return SLAM_OK;
    return slam_evidence_init_dev(pf->e, pf->map[pf->map_cur], pf->row_stride(), pf->Lp, pf->L, pf->n, pf->ev[pf->map_cur], pf->Lp,
                                  pf->prune_cmax);
}

// set_poses / set_map / reset discard the pending resample gather: nothing of it may run later
int drop_resample(slam_pf* pf)
{
    if (int rc = settle_means(pf)) return rc;   // without the gather every row is a current particle's
    pf->has_anc = false;
    pf->exchange_pending = false;
    if (pf->gated)   // ... and no weight is carried into the next frame
        if (int rc = slam_resample_gate_set(pf->e, pf->cfg.resample_ess_frac)) return rc;
    if (pf->comm) return comm_all_gather_finish(pf->comm);
    return SLAM_OK;
}

int create_common(slam_engine* e, const slam_pf_config* cfg, slam_comm* comm, int recv_capacity, slam_pf** out)
{
    if (!e || !cfg || !out || cfg->n_particles <= 0 || cfg->n_landmarks < 0 || !(cfg->meas_var > 0.0f) ||
        cfg->map_layout < SLAM_MAP_AUTO || cfg->map_layout > SLAM_MAP_SPLIT_PAGES)
        return SLAM_ERR_INVALID_ARG;

    *out = nullptr;
    if (e->live_sessions > 0) {   // the stages keep per-population state in the engine (gate, carried weights, exchange plan)
        snprintf(e->err, sizeof e->err, "this engine already runs a particle-filter session: one session per engine");
        return SLAM_ERR_NOT_READY;
    }
    if (comm && comm_engine(comm) != e) return SLAM_ERR_INVALID_ARG;
    if (int rc = slam_engine_sync(e)) return rc;   // also selects the engine's device
    slam_pf* pf = new (std::nothrow) slam_pf();
    if (!pf) return SLAM_ERR_HIP;
    pf->e = e;
    pf->cfg = *cfg;
    pf->n = cfg->n_particles;
    pf->L = cfg->n_landmarks;
    pf->Lp = (pf->L + 31) / 32 * 32;
    pf->comm = comm;
    if (comm) {
        pf->rank = comm_rank(comm);
        pf->world = comm_world(comm);
        pf->recv_cap = recv_capacity > 0 && recv_capacity < pf->n ? recv_capacity : pf->n;
    }
    pf->cap = pf->n + pf->recv_cap;
    pf->n_total = (int64_t)pf->n * pf->world;
    if (3 * pf->n_total > 0x7fffffff) {   // int32 ancestor indices into the all-gathered pose array
        delete pf;
        return SLAM_ERR_CAPACITY;
    }
    const size_t n = (size_t)pf->n, L = (size_t)pf->L, cap = (size_t)pf->cap, G = (size_t)pf->world;
    bool ok = true;
    // slam_pf_paged_set(e, 1) turns an AUTO request into PAGES (sessions made while it is set stay on pages)
    pf->layout_cfg = cfg->map_layout == SLAM_MAP_AUTO && e->pf_paged ? (int)SLAM_MAP_PAGES : cfg->map_layout;
    pf->paged = pf->L > 0 && (pf->layout_cfg == SLAM_MAP_PAGES || pf->layout_cfg == SLAM_MAP_SPLIT_PAGES);
    pf->nb = pf->Lp / kPageLandmarks;
    {
        const int64_t np = 2 * (int64_t)pf->cap * pf->nb;   // table rows (with the staging tail) never name more than half
        // page numbers are int32, and free_list_kernel's last tile may look 8191 past the end
        if (np > 0x7fffffff - 8192) {
            if (pf->paged) {
                delete pf;
                return SLAM_ERR_CAPACITY;
            }
            pf->auto_stuck = true;   // too many pages for this population: AUTO stays on rows
        }
        pf->npages = np > 0x7fffffff - 8192 ? 0 : (int)np;
        if (pf->nb < 2) pf->auto_stuck = true;   // one page per particle: nothing to gain from pages
    }
    pf->gated = cfg->resample_ess_frac > 0.0f && cfg->resample_ess_frac < 1.0f;
    if (L) ok = alloc_store(pf);
    // the split layout: asked for, or what AUTO keeps a session on while its frames observe most landmarks.  (Round 4 first kept
    // ESS-gated sessions on rows, whose update of a frame that keeps its population runs in place on the observed landmarks; the
    // split update of such a frame goes through the identity index out of place and is faster all the same: 65 536 x 500,
    // every landmark observed, 0.113 against 0.180 ms per frame; 32 observed on split pages 0.088 against 0.142-0.169.)
    const bool want_split = pf->layout_cfg == SLAM_MAP_SPLIT || pf->layout_cfg == SLAM_MAP_SPLIT_PAGES;
    if (L && ok && (want_split || pf->layout_cfg == SLAM_MAP_AUTO)) {
        const bool have = alloc_split_tables(pf);
        if (!have && want_split) ok = false;
        pf->split = have;
        if (have) place_split(pf, 0);
    }
    // survivor rows: a session that can have such frames (split — not pinned to split pages — on one GPU, resampling every frame,
    // the one-launch ancestor search); its buffers are made in front of the first such frame (survivor_buffers)
    pf->surv_can = L && ok && pf->split && !pf->paged && !comm && !pf->gated && cfg->resample_ess_frac <= 0.0f &&
                   ancestors_from_scan_fits(pf->n);
    if (L && ok && (pf->paged || (pf->layout_cfg == SLAM_MAP_AUTO && !pf->auto_stuck))) {
        ok = alloc_page_tables(pf);
        if (!ok && !pf->paged) {   // AUTO can live without them: it stays on rows
            pf->auto_stuck = true;
            ok = true;
        }
    }
    for (int b = 0; b < 2; ++b) {
        ok = ok && dev_alloc((void**)&pf->pose[b], 3 * n * 4) == hipSuccess;
        ok = ok && dev_alloc((void**)&pf->anc[b], n * 4) == hipSuccess;
        if (comm) ok = ok && dev_alloc((void**)&pf->pose_idx[b], n * 4) == hipSuccess;
    }
    ok = ok && dev_alloc((void**)&pf->score, n * 4) == hipSuccess && dev_alloc((void**)&pf->logw, n * 4) == hipSuccess &&
         dev_alloc((void**)&pf->count, n * 4) == hipSuccess && dev_alloc((void**)&pf->first, n * 4) == hipSuccess &&
         dev_alloc((void**)&pf->res_dev, kResBytes) == hipSuccess && dev_alloc((void**)&pf->sums_acc, 128) == hipSuccess &&
         dev_alloc((void**)&pf->moments_acc, 256) == hipSuccess && dev_alloc(&pf->res_all, kResBytes * G) == hipSuccess &&
         hipMemset(pf->sums_acc, 0, 128) == hipSuccess && hipMemset(pf->moments_acc, 0, 256) == hipSuccess;
    // results come back through the engine's mapped buffer (one session per engine; see engine_internal.h for why the
    // session does not allocate its own); the engine was drained above, so nothing of an earlier session writes to it any more
    pf->h_res = static_cast<decltype(pf->h_res)>(e->h_pf_res);
    pf->d_hres = static_cast<decltype(pf->d_hres)>(e->d_hpf_res);
    if (ok) memset(e->h_pf_res, 0, 128);
    if (comm)
        ok = ok && dev_alloc((void**)&pf->pose_all, 3 * n * G * 4) == hipSuccess &&
             dev_alloc((void**)&pf->pose_stage, 3 * cap * 4) == hipSuccess &&
             dev_alloc((void**)&pf->first_all, n * G * 4) == hipSuccess &&
             dev_alloc((void**)&pf->d_sum, 3 * 8) == hipSuccess && dev_alloc((void**)&pf->totals, 3 * 8 * G) == hipSuccess &&
             dev_alloc((void**)&pf->d_plan, 4 * SLAM_PLAN_WORDS(kMaxRanks)) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        slam_pf_destroy(pf);
        return SLAM_ERR_HIP;
    }
    if (comm)
        if (int rc = slam_exchange_set_capacity(e, pf->recv_cap)) {
            slam_pf_destroy(pf);
            return rc;
        }
    if (int rc = slam_resample_gate_set(e, pf->gated ? cfg->resample_ess_frac : 0.0f)) {
        slam_pf_destroy(pf);
        return rc;
    }
    const float origin[3] = { 0, 0, 0 };
    if (int rc = slam_pf_reset(pf, origin)) {   // a failed reset must not hand back a live object with an error code
        slam_pf_destroy(pf);
        return rc;
    }
    e->live_sessions++;
    pf->counted = true;
    *out = pf;
    return SLAM_OK;
}

}  // namespace
}  // namespace slam::session

using namespace slam;
using namespace slam::session;

extern "C" {

int slam_pf_create(slam_engine* e, const slam_pf_config* cfg, slam_pf** out)
{
    return create_common(e, cfg, nullptr, 0, out);
}

int slam_pf_create_sharded(slam_engine* e, const slam_pf_config* cfg, slam_comm* comm, int recv_capacity, slam_pf** out)
{
    if (!comm) return SLAM_ERR_INVALID_ARG;
    return create_common(e, cfg, comm, recv_capacity, out);
}

int slam_pf_destroy(slam_pf* pf)
{
    if (!pf) return SLAM_OK;
    (void)slam_engine_sync(pf->e);
    if (pf->counted) pf->e->live_sessions--;
    if (pf->comm) {
        (void)comm_all_gather_finish(pf->comm);
        (void)slam_engine_sync(pf->e);
        (void)slam_exchange_set_capacity(pf->e, 0);
    }
    if (pf->gated) (void)slam_resample_gate_set(pf->e, 0.0f);
    for (int b = 0; b < 2; ++b) {
        (void)hipFree(pf->pose[b]);
        (void)hipFree(pf->anc[b]);
        (void)hipFree(pf->pose_idx[b]);
    }
    if (pf->store) (void)hipFree(pf->store);
    if (pf->surv_store) (void)hipFree(pf->surv_store);
    if (pf->assoc_tab) (void)hipFree(pf->assoc_tab);   // (the stats live behind the table)
    if (pf->ev[0]) (void)hipFree(pf->ev[0]);           // (the second buffer and the stats live behind the first)
    if (pf->sight_spared) (void)hipFree(pf->sight_spared);
    if (pf->fov_outside) (void)hipFree(pf->fov_outside);
    if (pf->merge_stats) (void)hipFree(pf->merge_stats);
    if (pf->assoc_weight_missed) (void)hipFree(pf->assoc_weight_missed);   // (the terms live behind the misses)
    if (pf->known_prep) (void)hipFree(pf->known_prep);                      // (the map as it was given lives behind the prepared one)
    if (pf->known_stats) (void)hipFree(pf->known_stats);
    if (pf->known_missed) (void)hipFree(pf->known_missed);
    if (pf->known_ll) pf->e->ll_n = -1;
    free_page_tables(pf);
    free_split_tables(pf);
    for (void* p : { (void*)pf->score, (void*)pf->logw, (void*)pf->count, (void*)pf->first, (void*)pf->pose_all, (void*)pf->pose_stage, (void*)pf->first_all,
                     (void*)pf->d_sum, (void*)pf->totals, (void*)pf->d_plan, (void*)pf->sbuf,
                     (void*)pf->rbuf, (void*)pf->res_dev, (void*)pf->sums_acc, (void*)pf->moments_acc, pf->res_all })
        (void)hipFree(p);
    (void)hipFree(pf->sel);
    (void)hipFree(pf->conv_tmp);
    delete pf;   // h_res is the engine's
    return SLAM_OK;
}

int slam_pf_reset(slam_pf* pf, const float pose[3])
{
    if (!pf || !pose) return SLAM_ERR_INVALID_ARG;
    const size_t n = (size_t)pf->n;
    std::vector<float> h(3 * n);
    for (int k = 0; k < 3; ++k)
        for (size_t i = 0; i < n; ++i) h[k * n + i] = pose[k];
    if (int rc = drop_resample(pf)) return rc;
    if (int rc = slam_engine_sync(pf->e)) return rc;
    if (hipMemcpy(pf->pose[pf->cur], h.data(), 3 * n * 4, hipMemcpyHostToDevice) != hipSuccess) return SLAM_ERR_HIP;
    if (pf->split) {   // every landmark of every particle "not seen yet": one class
        split_new_epoch(pf);
        SLAM_HIP_TRY(pf->e, launch_split_reset(pf->e->stream, pf->mean[pf->sp_cur], class_store(pf), pf->n, dev_word(pf, RES_LIVE),
                                               pf->cls_epoch));
    }
    if (pf->paged)   // every particle names ONE shared page of landmarks not seen yet (split pages: of zero means), the rest of the pool is free
        SLAM_HIP_TRY(pf->e, launch_pages_reset(pf->e->stream, page_pool(pf), (int64_t)pf->n * pf->nb));
    if (pf->split || pf->paged) {
        if (int rc = slam_engine_sync(pf->e)) return rc;
    } else if (pf->L) {   // rows: P_xx = -1: "not seen yet"
        const size_t Lp = (size_t)pf->Lp;
        std::vector<float> row(5 * Lp, 0.0f);
        for (size_t l = 0; l < Lp; ++l) row[2 * Lp + l] = -1.0f;
        // one row on the host, replicated over the particles in chunks (a 52 GB map does not pass through host memory)
        const size_t chunk = n < 4096 ? n : 4096;
        std::vector<float> m(5 * Lp * chunk);
        for (size_t i = 0; i < chunk; ++i) memcpy(&m[i * 5 * Lp], row.data(), 5 * Lp * 4);
        for (size_t i0 = 0; i0 < n; i0 += chunk) {
            const size_t k = n - i0 < chunk ? n - i0 : chunk;
            if (hipMemcpy(pf->map[pf->map_cur] + i0 * 5 * Lp, m.data(), k * 5 * Lp * 4, hipMemcpyHostToDevice) != hipSuccess)
                return SLAM_ERR_HIP;
        }
    }
    pf->frame = 0;
    return evidence_from_maps(pf);   // (pruning: every slot unseen, every evidence byte 0)
}

int slam_pf_set_poses_host(slam_pf* pf, const float* x, const float* y, const float* theta)
{
    if (!pf || !x || !y || !theta) return SLAM_ERR_INVALID_ARG;
    const size_t n = (size_t)pf->n;
    if (int rc = drop_resample(pf)) return rc;
    if (int rc = slam_engine_sync(pf->e)) return rc;
    float* d = pf->pose[pf->cur];
    if (hipMemcpy(d, x, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + n, y, n * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(d + 2 * n, theta, n * 4, hipMemcpyHostToDevice) != hipSuccess)
        return SLAM_ERR_HIP;
    return SLAM_OK;
}

int slam_pf_set_map_host(slam_pf* pf, const float* rows)
{
    if (!pf || !rows || !pf->L) return SLAM_ERR_INVALID_ARG;
    if (int rc = settle_means(pf)) return rc;
    if (int rc = slam_engine_sync(pf->e)) return rc;
    if (pf->has_anc) return SLAM_ERR_NOT_READY;   // set poses / reset first: a gather is pending
    // host [n][5][L] -> device [n][5][Lp]: 5n planes of L floats each
    const bool indirect = pf->paged || pf->split;   // no rows to copy into: a scratch copy goes through slam_pf_set_map_dev
    float* dense = indirect ? nullptr : pf->map[pf->map_cur];
    if (indirect && hipMalloc((void**)&dense, (size_t)pf->row_stride() * pf->n * 4) != hipSuccess) return SLAM_ERR_HIP;
    int rc = SLAM_OK;
    if (hipMemcpy2D(dense, (size_t)pf->Lp * 4, rows, (size_t)pf->L * 4, (size_t)pf->L * 4, 5 * (size_t)pf->n,
                    hipMemcpyHostToDevice) != hipSuccess)
        rc = SLAM_ERR_HIP;
    if (indirect) {
        if (rc == SLAM_OK) rc = slam_pf_set_map_dev(pf, dense, pf->row_stride(), pf->Lp);
        if (rc == SLAM_OK) rc = slam_engine_sync(pf->e);
        (void)hipFree(dense);
    } else if (rc == SLAM_OK) {
        rc = evidence_from_maps(pf);   // (pruning: the loaded maps are trusted)
    }
    return rc;
}

int slam_pf_set_map_dev(slam_pf* pf, const float* d_rows, int64_t row_stride, int plane_stride)
{
    if (!pf || !d_rows || !pf->L || plane_stride < pf->L || row_stride < 5 * (int64_t)plane_stride) return SLAM_ERR_INVALID_ARG;
    if (int rc = settle_means(pf)) return rc;
    if (pf->has_anc) return SLAM_ERR_NOT_READY;   // set poses / reset first: a gather is pending
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (pf->split && pf->paged) {   // split pages: classes and mean rows first, then the means onto pages
        pf->paged = false;
        pf->sp_cur = 0;
        if (int rc = split_from_rows(pf, d_rows, row_stride, plane_stride, pf->n)) return rc;
        return split_means_to_pages(pf);
    }
    if (pf->split) return split_from_rows(pf, d_rows, row_stride, plane_stride, pf->n);
    if (pf->paged) {
        SLAM_HIP_TRY(e, launch_pages_from_rows(e->stream, d_rows, row_stride, plane_stride, pf->L, pf->n, page_pool(pf)));
        return SLAM_OK;
    }
    for (int pl = 0; pl < 5; ++pl)   // plane by plane: one 2-D copy each whatever the caller's row stride is
        SLAM_HIP_TRY(e, hipMemcpy2DAsync(pf->map[pf->map_cur] + (size_t)pl * pf->Lp, (size_t)pf->row_stride() * 4,
                                         d_rows + (size_t)pl * plane_stride, (size_t)row_stride * 4, (size_t)pf->L * 4,
                                         (size_t)pf->n, hipMemcpyDeviceToDevice, e->stream));
    return evidence_from_maps(pf);   // (pruning: the loaded maps are trusted)
}

int slam_pf_refine_set(slam_pf* pf, float step_xy, float step_theta, int sweeps)
{
    if (!pf || sweeps < 0 || sweeps > 16) return SLAM_ERR_INVALID_ARG;
    if (sweeps > 0 && !(step_xy >= 0.0f && step_theta >= 0.0f && step_xy <= FLT_MAX && step_theta <= FLT_MAX)) return SLAM_ERR_INVALID_ARG;
    pf->refine_step_xy = sweeps ? step_xy : 0.0f;
    pf->refine_step_theta = sweeps ? step_theta : 0.0f;
    pf->refine_sweeps = sweeps;
    return SLAM_OK;
}

int slam_pf_meas_cov_set(slam_pf* pf, const float meas_cov[3])
{
    if (!pf || !meas_cov) return SLAM_ERR_INVALID_ARG;
    if (pf->layout_cfg != SLAM_MAP_ROWS || pf->L == 0) {
        snprintf(pf->e->err, sizeof pf->e->err, "a 2x2 measurement covariance makes the landmark covariances per particle: that needs the "
                                                "row layout (map_layout = SLAM_MAP_ROWS, n_landmarks > 0)");
        return SLAM_ERR_INVALID_ARG;
    }
    EkfAnisoCov q;
    if (!slam_aniso_cov_from(pf->e, meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    const bool iso = pf->is_meas_var(meas_cov);
    if (pf->assoc_on && !iso) {
        snprintf(pf->e->err, sizeof pf->e->err, "data association is on (slam_pf_assoc_set): it gates with meas_var * I, a 2x2 "
                                                "measurement covariance cannot be set (slam_pf_assoc_cov_set sets covariance and "
                                                "gates together)");
        return SLAM_ERR_INVALID_ARG;
    }
    for (int k = 0; k < 3; ++k) pf->meas_cov[k] = meas_cov[k];
    // {meas_var, 0, meas_var}: the session's own isotropic update again, exactly as without this call
    pf->aniso = !iso;
    return SLAM_OK;
}

int slam_pf_assoc_set(slam_pf* pf, float gate, float new_gate, int create)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (gate == 0.0f) {   // off: the session runs exactly what it ran before the first call (pruning and the detector go off with it)
        pf->assoc_on = false;
        pf->assoc_aniso = false;
        pf->assoc_detcov = false;
        pf->prune_on = false;
        pf->sight_bins = 0;
        pf->fov_on = false;
        pf->merge_gate = 0.0f;
        pf->assoc_weight_on = false;
        pf->detect_on = false;
        pf->detect_fit_on = false;
        pf->detect_noise_on = false;
        return SLAM_OK;
    }
    if (pf->layout_cfg != SLAM_MAP_ROWS || pf->L == 0 || pf->comm) {
        snprintf(e->err, sizeof e->err, "data association gives every particle its own observed landmarks: that needs the row "
                                        "layout on one GPU (map_layout = SLAM_MAP_ROWS, n_landmarks > 0, not sharded)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (pf->aniso) {
        snprintf(e->err, sizeof e->err, "data association gates with meas_var * I: not while a 2x2 measurement covariance is in "
                                        "force (slam_pf_meas_cov_set)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!(gate > 0.0f && gate <= FLT_MAX) || !(new_gate >= gate) || (create != 0 && create != 1) || pf->L > SLAM_MAX_OBS) {
        snprintf(e->err, sizeof e->err, "association needs a finite gate > 0, new_gate >= gate, create in {0, 1} and at most %d landmarks",
                 (int)SLAM_MAX_OBS);
        return SLAM_ERR_INVALID_ARG;
    }
    if (!pf->assoc_tab) {
        SLAM_HIP_TRY(e, hipSetDevice(e->device));
        const size_t tab = pf->byte_table(), st = (size_t)pf->n * 3 * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->assoc_tab, tab + st));   // one allocation: the table, then the stats
        pf->assoc_stats = reinterpret_cast<int32_t*>(pf->assoc_tab + tab);
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->assoc_tab, SLAM_ASSOC_NONE, tab, e->stream));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->assoc_stats, 0, st, e->stream));
    }
    pf->assoc_on = true;
    pf->assoc_aniso = false;   // (slam_pf_assoc_cov_set behind this call says otherwise)
    pf->assoc_detcov = false;  // (slam_pf_assoc_detcov_set likewise)
    pf->assoc_gate = gate;
    pf->assoc_new_gate = new_gate;
    pf->assoc_create = create;
    return SLAM_OK;
}

int slam_pf_assoc_cov_set(slam_pf* pf, const float meas_cov[3], float gate, float new_gate, int create)
{
    if (!pf || !meas_cov) return SLAM_ERR_INVALID_ARG;
    EkfAnisoCov q;
    if (!slam_aniso_cov_from(pf->e, meas_cov, &q)) return SLAM_ERR_INVALID_ARG;
    if (gate == 0.0f) {   // slam_pf_assoc_set(0, ..) is the switch-off: here a gate has to be given
        snprintf(pf->e->err, sizeof pf->e->err, "association needs a finite gate > 0 (slam_pf_assoc_set(0, ..) switches it off)");
        return SLAM_ERR_INVALID_ARG;
    }
    // the conditions, the refusals and the table of the isotropic switch; a refused call leaves the session as it was
    if (int rc = slam_pf_assoc_set(pf, gate, new_gate, create)) return rc;
    // {meas_var, 0, meas_var}: exactly slam_pf_assoc_set — the isotropic kernels, the same bits
    for (int k = 0; k < 3; ++k) pf->assoc_cov[k] = meas_cov[k];
    pf->assoc_aniso = !pf->is_meas_var(meas_cov);
    return SLAM_OK;
}

int slam_pf_assoc_detcov_set(slam_pf* pf, float gate, float new_gate, int create)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    if (gate == 0.0f) {   // slam_pf_assoc_set(0, ..) is the switch-off: here a gate has to be given
        snprintf(pf->e->err, sizeof pf->e->err, "association needs a finite gate > 0 (slam_pf_assoc_set(0, ..) switches it off)");
        return SLAM_ERR_INVALID_ARG;
    }
    // the conditions, the refusals and the table of the isotropic switch; a refused call leaves the session as it was
    if (int rc = slam_pf_assoc_set(pf, gate, new_gate, create)) return rc;
    pf->assoc_detcov = true;
    return SLAM_OK;
}

int slam_pf_prune_set(slam_pf* pf, int hit, int miss, int cmax, float view_range)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (hit == 0) {   // off: the session runs exactly what it ran before the first call
        pf->prune_on = false;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (which is what every layout but rows, a sharded session and a 2x2 covariance come down to)
        snprintf(e->err, sizeof e->err, "pruning reads the frame's association table: it needs data association switched on "
                                        "(slam_pf_assoc_set: the row layout on one GPU, not sharded, meas_var * I)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (hit < 1 || hit > 255 || miss < 1 || miss > 255 || cmax < 1 || cmax > 255 || !(view_range > 0.0f && view_range <= FLT_MAX)) {
        snprintf(e->err, sizeof e->err, "pruning needs hit, miss and cmax in 1 .. 255 and a finite view_range > 0");
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->ev[0]) {   // once, at the switch: two evidence buffers, then the stats — device memory only
        const size_t buf = pf->byte_table(), st = (size_t)pf->n * 2 * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->ev[0], 2 * buf + st));
        pf->ev[1] = pf->ev[0] + buf;
        pf->ev_stats = reinterpret_cast<int32_t*>(pf->ev[1] + buf);
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->ev[0], 0, 2 * buf + st, e->stream));
    }
    pf->prune_on = true;
    pf->prune_hit = hit;
    pf->prune_miss = miss;
    pf->prune_cmax = cmax;
    pf->prune_range = view_range;
    return evidence_from_maps(pf);   // the current maps are trusted (indexed like them: before the pending gather)
}

int slam_pf_prune_sight_set(slam_pf* pf, int bins, float margin)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (bins == 0) {   // off: the evidence stage the session ran before the first call
        pf->sight_bins = 0;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (accepted where slam_pf_prune_set is)
        snprintf(e->err, sizeof e->err, "line of sight belongs to the pruning of an associating session: it needs data association "
                                        "switched on (slam_pf_assoc_set: the row layout on one GPU, not sharded, meas_var * I)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!sight_bins_ok(bins) || !(margin > 0.0f && margin <= FLT_MAX)) {
        snprintf(e->err, sizeof e->err, "line of sight needs bins a power of two in %d .. %d and a finite margin > 0", kSightMinBins, kSightMaxBins);
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->sight_spared) {   // once, at the switch — never inside a frame: the counts, and the engine's table
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->sight_spared, (size_t)pf->n * sizeof(int32_t)));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->sight_spared, 0, (size_t)pf->n * sizeof(int32_t), e->stream));
    }
    if (!e->sight_buf.p) SLAM_HIP_TRY(e, e->sight_buf.ensure(sizeof(float) * kSightMaxBins));
    pf->sight_bins = bins;
    pf->sight_margin = margin;
    return SLAM_OK;
}

int slam_pf_prune_fov_set(slam_pf* pf, int on, float angle_min, float angle_max, float edge)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (!on) {   // off: the evidence stage the session ran before the first call
        pf->fov_on = false;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (accepted where slam_pf_prune_sight_set is)
        snprintf(e->err, sizeof e->err, "a field of view belongs to the pruning of an associating session: it needs data association "
                                        "switched on (slam_pf_assoc_set: the row layout on one GPU, not sharded, meas_var * I)");
        return SLAM_ERR_INVALID_ARG;
    }
    const float pi = 3.14159274f;   // float32 pi
    const float from = angle_min + edge, to = angle_max - edge;   // (a NaN or an infinity anywhere fails a comparison below)
    if (!(edge >= 0.0f && edge <= FLT_MAX && angle_min >= -pi && angle_max <= pi && from < to)) {
        snprintf(e->err, sizeof e->err, "a field of view needs finite angles -pi <= angle_min, angle_max <= pi and a finite edge >= 0 "
                                        "with angle_min + edge < angle_max - edge");
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->fov_outside) {   // once, at the switch — never inside a frame
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->fov_outside, (size_t)pf->n * sizeof(int32_t)));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->fov_outside, 0, (size_t)pf->n * sizeof(int32_t), e->stream));
    }
    pf->fov_lo = slam_fov_bound(from);
    pf->fov_hi = slam_fov_bound(to);
    pf->fov_on = true;
    return SLAM_OK;
}

int slam_pf_merge_set(slam_pf* pf, float merge_gate)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (merge_gate == 0.0f) {   // off: the session runs exactly what it ran before the first call
        pf->merge_gate = 0.0f;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (accepted where slam_pf_prune_set is; under any of the three noise forms)
        snprintf(e->err, sizeof e->err, "merging reads the frame's association table: it needs data association switched on "
                                        "(slam_pf_assoc_set: the row layout on one GPU, not sharded)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!(merge_gate > 0.0f && merge_gate <= FLT_MAX)) {
        snprintf(e->err, sizeof e->err, "merging needs a finite merge_gate > 0 (0 switches it off)");
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->merge_stats) {   // once, at the switch — never inside a frame
        const size_t st = (size_t)pf->n * 3 * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->merge_stats, st));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->merge_stats, 0, st, e->stream));
    }
    pf->merge_gate = merge_gate;
    return SLAM_OK;
}

int slam_pf_assoc_weight_set(slam_pf* pf, float log_new, float log_clutter, float log_miss, int on)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (!on) {   // off: the session runs exactly what it ran before the first call
        pf->assoc_weight_on = false;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (accepted where slam_pf_merge_set is; under any of the three noise forms)
        snprintf(e->err, sizeof e->err, "weighing what the association leaves unexplained reads the frame's association stats: it needs data "
                                        "association switched on (slam_pf_assoc_set: the row layout on one GPU, not sharded)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!assoc_weight_const_ok(log_new) || !assoc_weight_const_ok(log_clutter) || !assoc_weight_const_ok(log_miss)) {
        snprintf(e->err, sizeof e->err, "log_new, log_clutter and log_miss are log-likelihoods of events: each must be finite and <= 0");
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->assoc_weight_missed) {   // once, at the switch — never inside a frame
        const size_t bytes = (size_t)pf->n * (sizeof(int32_t) + sizeof(float));
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->assoc_weight_missed, bytes));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->assoc_weight_missed, 0, bytes, e->stream));
        pf->assoc_weight_terms = reinterpret_cast<float*>(pf->assoc_weight_missed + pf->n);
    }
    pf->assoc_weight_log[0] = log_new;
    pf->assoc_weight_log[1] = log_clutter;
    pf->assoc_weight_log[2] = log_miss;
    pf->assoc_weight_on = true;
    return SLAM_OK;
}

int slam_pf_detect_set(slam_pf* pf, const slam_detect_params* params) { return slam_pf_detect_fit_set(pf, params, nullptr); }

// fit == nullptr: the centroid detector (slam_pf_detect_set); a refused call leaves the session as it was
int slam_pf_detect_fit_set(slam_pf* pf, const slam_detect_params* params, const slam_detect_fit* fit)
{
    return slam_pf_detect_noise_set(pf, params, fit, nullptr);
}

// noise == nullptr: the detector without the model (slam_pf_detect_fit_set); a refused call leaves the session as it was
int slam_pf_detect_noise_set(slam_pf* pf, const slam_detect_params* params, const slam_detect_fit* fit, const slam_detect_noise* noise)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (!params) {   // off: the session runs exactly what it ran before the first call
        pf->detect_on = false;
        pf->detect_fit_on = false;
        pf->detect_noise_on = false;
        return SLAM_OK;
    }
    if (!pf->assoc_on && !pf->known_on) {   // (which is what every layout but rows, a sharded session and a 2x2 covariance come down to)
        snprintf(e->err, sizeof e->err, "the detector makes the detections the association reads: it needs data association switched "
                                        "on (slam_pf_assoc_set: the row layout on one GPU, not sharded, meas_var * I) or a known map "
                                        "(slam_pf_known_map_set)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (pf->known_on && !pf->known_detcov && noise) {
        snprintf(e->err, sizeof e->err, "localisation in a known map weighs with meas_var * I: the detector's noise model cannot be "
                                        "switched on (slam_pf_detect_set / slam_pf_detect_fit_set)");
        return SLAM_ERR_INVALID_ARG;
    }
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
    pf->detect_on = true;
    pf->detect_params = *params;
    pf->detect_fit_on = fit != nullptr;
    if (fit) pf->detect_fit = *fit;
    pf->detect_noise_on = noise != nullptr;
    if (noise) pf->detect_noise = *noise;
    return SLAM_OK;
}

// detcov: the stage under the detections' own covariances (slam_pf_known_map_detcov_set) — nothing is prepared, meas_var is not read
static int known_map_set(slam_pf* pf, const float* rows, int nlandmarks, float gate, float log_clutter, bool detcov)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (!rows) {   // off: the session runs exactly what it ran before the first call (the detector goes off with it)
        if (pf->known_on) {
            pf->detect_on = false;
            pf->detect_fit_on = false;
            pf->detect_noise_on = false;
        }
        if (pf->known_ll) e->ll_n = -1;   // (the stage's log-likelihoods are nobody's any more)
        pf->known_ll = false;
        pf->known_on = false;
        pf->known_detcov = false;
        pf->known_miss_on = false;   // (the misses go off with the map; replacing the map keeps them)
        return SLAM_OK;
    }
    if (pf->L != 0 || pf->comm) {
        snprintf(e->err, sizeof e->err, "localisation in a known map is for a session without maps of its own on one GPU "
                                        "(n_landmarks == 0, not sharded)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (nlandmarks < 1 || nlandmarks > SLAM_MAX_OBS || !(gate > 0.0f && gate <= FLT_MAX) || !assoc_weight_const_ok(log_clutter)) {
        snprintf(e->err, sizeof e->err, "a known map needs 1 .. %d landmarks, a finite gate > 0 and a finite log_clutter <= 0", (int)SLAM_MAX_OBS);
        return SLAM_ERR_INVALID_ARG;
    }
    const size_t L = (size_t)nlandmarks, Lp = (L + 31) / 32 * 32;
    const float q = pf->cfg.meas_var;
    for (size_t k = 0; k < 5 * L; ++k)
        if (!(rows[k] >= -FLT_MAX && rows[k] <= FLT_MAX)) {   // (NaN fails every comparison)
            snprintf(e->err, sizeof e->err, "known map: value %zu of plane %zu is not finite", k % L, k / L);
            return SLAM_ERR_INVALID_ARG;
        }
    for (size_t l = 0; l < L; ++l) {
        const float pxx = rows[2 * L + l], pxy = rows[3 * L + l], pyy = rows[4 * L + l];
        if (pxx < 0.0f) continue;   // the slot holds no landmark
        if (detcov) {   // P alone: every Q_k is positive definite, so P + R_w is wherever P is positive semi-definite
            if (!(pyy >= 0.0f && pxx * pyy - pxy * pxy >= 0.0f)) {
                snprintf(e->err, sizeof e->err, "known map: landmark %zu has no positive semi-definite P", l);
                return SLAM_ERR_INVALID_ARG;
            }
            continue;
        }
        const float a = pxx + q, c = pyy + q;
        const float det = a * c - pxy * pxy;   // (the prepare kernel's own operations)
        if (!(a > 0.0f && c > 0.0f && det > 0.0f)) {
            snprintf(e->err, sizeof e->err, "known map: landmark %zu has no positive definite P + meas_var * I", l);
            return SLAM_ERR_INVALID_ARG;
        }
    }
    // ---- accepted: everything the frames need is made here, never inside a frame
    if (int rc = slam_engine_sync(e)) return rc;   // (a frame in flight may still read the map that is replaced; also selects the device)
    if (11 * Lp > pf->known_cap) {
        float* fresh = nullptr;
        SLAM_HIP_TRY(e, dev_alloc((void**)&fresh, 11 * Lp * sizeof(float)));
        if (pf->known_prep) (void)hipFree(pf->known_prep);
        pf->known_prep = fresh;
        pf->known_cap = 11 * Lp;
        pf->known_on = false;   // (the old map is gone: until the new one is prepared below there is none)
    }
    if (!pf->known_stats) {
        const size_t st = (size_t)pf->n * 3 * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->known_stats, st));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->known_stats, 0, st, e->stream));
    }
    SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)pf->n));
    std::vector<float> h(5 * Lp, 0.0f);
    for (size_t l = 0; l < Lp; ++l) h[2 * Lp + l] = -1.0f;   // padding: slots that hold no landmark
    for (int p = 0; p < 5; ++p) memcpy(&h[(size_t)p * Lp], rows + (size_t)p * L, L * sizeof(float));
    float* raw = pf->known_prep + 6 * Lp;
    pf->known_on = false;
    SLAM_HIP_TRY(e, hipMemcpy(raw, h.data(), 5 * Lp * sizeof(float), hipMemcpyHostToDevice));
    if (!detcov)
        if (int rc = slam_known_map_prepare_dev(e, raw, (int)Lp, nlandmarks, q, pf->known_prep)) return rc;
    if (!detcov && pf->detect_noise_on) pf->detect_noise_on = false;   // (this form takes no model: the detector goes on without it)
    pf->known_detcov = detcov;
    pf->known_L = nlandmarks;
    pf->known_Lp = (int)Lp;
    pf->known_gate = gate;
    pf->known_log_clutter = log_clutter;
    pf->known_on = true;
    return SLAM_OK;
}

int slam_pf_known_map_set(slam_pf* pf, const float* rows, int nlandmarks, float gate, float log_clutter)
{
    return known_map_set(pf, rows, nlandmarks, gate, log_clutter, false);
}

int slam_pf_known_map_detcov_set(slam_pf* pf, const float* rows, int nlandmarks, float gate, float log_clutter)
{
    return known_map_set(pf, rows, nlandmarks, gate, log_clutter, true);
}

int slam_pf_known_map_miss_set(slam_pf* pf, float log_miss, float view_range, int fov_on, float angle_min, float angle_max, float edge,
                               int sight_bins, float margin)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (view_range == 0.0f) {   // off: the session runs exactly what it ran before the first call
        pf->known_miss_on = false;
        return SLAM_OK;
    }
    if (!pf->known_on) {
        snprintf(e->err, sizeof e->err, "the misses of localisation are counted against a known map: it needs one set "
                                        "(slam_pf_known_map_set or slam_pf_known_map_detcov_set)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!assoc_weight_const_ok(log_miss) || !(view_range > 0.0f && view_range <= FLT_MAX)) {
        snprintf(e->err, sizeof e->err, "the misses of localisation need a finite log_miss <= 0 and a finite view_range > 0 (0 switches them off)");
        return SLAM_ERR_INVALID_ARG;
    }
    const float pi = 3.14159274f;   // float32 pi
    const float from = angle_min + edge, to = angle_max - edge;   // (a NaN or an infinity anywhere fails a comparison below)
    if (fov_on && !(edge >= 0.0f && edge <= FLT_MAX && angle_min >= -pi && angle_max <= pi && from < to)) {   // as slam_pf_prune_fov_set
        snprintf(e->err, sizeof e->err, "a field of view needs finite angles -pi <= angle_min, angle_max <= pi and a finite edge >= 0 "
                                        "with angle_min + edge < angle_max - edge");
        return SLAM_ERR_INVALID_ARG;
    }
    if (sight_bins != 0 && (!sight_bins_ok(sight_bins) || !(margin > 0.0f && margin <= FLT_MAX))) {   // as slam_pf_prune_sight_set
        snprintf(e->err, sizeof e->err, "line of sight needs bins a power of two in %d .. %d and a finite margin > 0", kSightMinBins, kSightMaxBins);
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (!pf->known_missed) {   // once, at the switch — never inside a frame: the counts, and the engine's table
        const size_t bytes = 3 * (size_t)pf->n * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->known_missed, bytes));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->known_missed, 0, bytes, e->stream));
    }
    if (sight_bins != 0 && !e->sight_buf.p) SLAM_HIP_TRY(e, e->sight_buf.ensure(sizeof(float) * kSightMaxBins));
    pf->known_log_miss = log_miss;
    pf->known_view.view_range = view_range;
    pf->known_view.lo = fov_on ? slam_fov_bound(from) : 0.0f;
    pf->known_view.hi = fov_on ? slam_fov_bound(to) : 4.0f;
    pf->known_view.sight = sight_bins != 0;
    pf->known_view.margin = sight_bins != 0 ? margin : 0.0f;
    pf->known_sight_bins = sight_bins;
    pf->known_miss_on = true;
    return SLAM_OK;
}

int slam_pf_known_map_miss_device_view(slam_pf* pf, const int32_t** missed, const int32_t** spared, const int32_t** outside)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    if (!pf->known_missed) return SLAM_ERR_NOT_READY;   // slam_pf_known_map_miss_set never switched the misses on
    if (missed) *missed = pf->known_missed;
    if (spared) *spared = pf->known_missed + (size_t)pf->n;
    if (outside) *outside = pf->known_missed + 2 * (size_t)pf->n;
    return SLAM_OK;
}

int slam_pf_known_map_device_view(slam_pf* pf, const float** prepared, int32_t* nlandmarks, const int32_t** stats)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    if (!pf->known_stats) return SLAM_ERR_NOT_READY;
    if (prepared) *prepared = pf->known_on && !pf->known_detcov ? pf->known_prep : nullptr;
    if (nlandmarks) *nlandmarks = pf->known_on ? pf->known_L : 0;
    if (stats) *stats = pf->known_stats;
    return SLAM_OK;
}

// The pending resample and the proposals in ONE launch: pose[cur] through anc[cur] -> the other pose buffer, which becomes the
// current one.  The counts come back through the mapped result block; nothing else is waited for.  pair == nullptr: proposals
// from single detections (two counts, min_det 1); else from detection pairs under pair = {tol, min_sep} (four counts, min_det 2).
static int known_map_reseed(slam_pf* pf, float fraction, const float* pair, int32_t* counts)
{
    if (!pf || !counts) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (pf->comm || pf->L > 0 || !pf->known_on) {
        snprintf(e->err, sizeof e->err, "reseeding draws its proposals from a known map: %s",
                 pf->comm ? "a sharded session cannot have one" : pf->L > 0 ? "a session with n_landmarks > 0 cannot have one"
                                                                           : "the mode is off (slam_pf_known_map_set or slam_pf_known_map_detcov_set)");
        return SLAM_ERR_NOT_READY;
    }
    if (!(fraction > 0.0f && fraction <= 1.0f)) {   // (NaN fails every comparison)
        snprintf(e->err, sizeof e->err, "reseed: the fraction must lie in (0, 1]");
        return SLAM_ERR_INVALID_ARG;
    }
    if (pair && (!(pair[0] >= 0.0f) || !(pair[1] > pair[0]) || !isfinite(pair[1]) || pf->known_L < 2)) {
        snprintf(e->err, sizeof e->err, "reseed from pairs: 0 <= tol < min_sep, both finite, and a map of two landmarks or more");
        return SLAM_ERR_INVALID_ARG;
    }
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (e->ndet < 0) {
        snprintf(e->err, sizeof e->err, "reseed: no detections were handed over");
        return SLAM_ERR_NOT_READY;
    }
    const int ncounts = pair ? 4 : 2;
    const ResWord words = pair ? RES_RESEED_PAIRS : RES_RESEED;
    for (int k = 0; k < ncounts; ++k) counts[k] = 0;
    if (e->ndet < (pair ? 2 : 1)) return SLAM_OK;   // nothing to propose from: the session is as it was
    if (pf->gated && pf->has_anc) {     // the verdict of the last frame, before the gate forgets it below
        int resampled = 1;
        if (int rc = slam_resample_happened_host(e, &resampled)) return rc;
        pf->frames_resampled += resampled ? 1 : 0;
    }
    const size_t sn = (size_t)pf->n;
    const float* src = pf->pose[pf->cur];
    float* dst = pf->pose[1 - pf->cur];
    const float* map = pf->known_prep + 6 * (size_t)pf->known_Lp;
    const int32_t* anc = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    const uint32_t seq = ++pf->res_seq;
    const slam_reseed_mapped mapped{ dev_word(pf, words), reinterpret_cast<uint32_t*>(dev_word(pf, RES_SEQ)), seq };
    bool launched = false;
    if (int rc = pair ? slam_engine_pose_reseed_pairs(e, map, pf->known_Lp, pf->known_L, src, src + sn, src + 2 * sn, anc, dst, dst + sn,
                                                      dst + 2 * sn, pf->n, 0, pf->cfg.seed, pf->frame, fraction, pair[0], pair[1], nullptr,
                                                      &mapped, nullptr, &launched)
                      : slam_engine_pose_reseed(e, map, pf->known_Lp, pf->known_L, src, src + sn, src + 2 * sn, anc, dst, dst + sn,
                                                dst + 2 * sn, pf->n, 0, pf->cfg.seed, pf->frame, fraction, nullptr, &mapped, nullptr, &launched))
        return rc;
    pf->cur = 1 - pf->cur;
    pf->has_anc = false;
    pf->reseeded = true;
    if (pf->gated)   // no weight is carried into the next frame
        if (int rc = slam_resample_gate_set(e, pf->cfg.resample_ess_frac)) return rc;
    const volatile uint32_t* h_seq = reinterpret_cast<const volatile uint32_t*>(host_word(pf, RES_SEQ));
    if (int rc = slam_engine_wait_flag(e, nullptr, h_seq, seq, "reseed flag")) return rc;
    for (int k = 0; k < ncounts; ++k) counts[k] = host_word(pf, words)[k];
    return SLAM_OK;
}

int slam_pf_known_map_reseed(slam_pf* pf, float fraction, int32_t counts[2]) { return known_map_reseed(pf, fraction, nullptr, counts); }

int slam_pf_known_map_reseed_pairs(slam_pf* pf, float fraction, float tol, float min_sep, int32_t counts[4])
{
    const float pair[2] = { tol, min_sep };
    return known_map_reseed(pf, fraction, pair, counts);
}

int slam_pf_rows_received(const slam_pf* pf) { return pf ? pf->rows_received : 0; }
int64_t slam_pf_frames_resampled(const slam_pf* pf) { return pf ? pf->frames_resampled : 0; }
int64_t slam_pf_layout_changes(const slam_pf* pf) { return pf ? pf->conversions : 0; }
}  // extern "C"
