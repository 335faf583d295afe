// pf_session_frame.hip — one frame of a session (slam_pf_step): what the frame is (frame_facts), the arguments its launches
// take, and its stages in the order they are issued — front launch, resample gate and exchange between the ranks (migrate),
// the landmark update per storage form, weights and scan, resample.

#include <stdio.h>
#include <stdlib.h>

#include "pf_session.h"

namespace slam::session {
namespace {

// The classes' update of a frame (cov_update_body.h), in place, once per class still in use; nlandmarks = 0: only the list of
// classes in use is brought up to date (a frame without observations).  The launch is as wide as the host knows the list to
// be at most: its length as of some earlier launch (mapped memory, read without waiting) plus the classes that arrived since
// (sharded sessions) — the second word is the running count of arrivals as of that launch; it is read FIRST and written
// last, so a torn pair only over-estimates; before anything of this epoch has arrived: every class there can be.
// Gives the arguments and the width, and moves the bookkeeping on as if it had been launched: the weights' launch carries it
// (weights_with_classes), or the scan's on a frame whose front launch made the weights (update_split, scan_stage).
void split_class_prepare(slam_pf* pf, int nlandmarks, bool save_prior, CovArgs& ca, int& bound)
{
    ca.save_cov = save_prior ? pf->save_cov : nullptr;
    ca.save_covx = save_prior ? pf->save_covx : nullptr;
    const uint64_t hm = __atomic_load_n(reinterpret_cast<const uint64_t*>(host_word(pf, RES_CLS_MARK)), __ATOMIC_ACQUIRE),
                   hl = __atomic_load_n(reinterpret_cast<const uint64_t*>(host_word(pf, RES_LIVE)), __ATOMIC_ACQUIRE);
    const bool fresh = (uint32_t)(hl >> 32) == pf->cls_epoch && (uint32_t)hl > 0;
    const uint32_t mark = (uint32_t)(hm >> 32) == pf->cls_epoch ? (uint32_t)hm : 0u;   // (no launch of this epoch has said yet: 0)
    const int64_t upper = fresh ? (int64_t)(uint32_t)hl + (int64_t)(pf->cls_appended - mark) : (int64_t)pf->cap;
    bound = upper < pf->cap ? (int)upper : pf->cap;
    ca.cov = pf->cov;
    ca.cov_stride = pf->cov_stride();
    ca.covx = pf->covx;
    ca.covx_stride = pf->mean_stride();
    ca.plane_stride = pf->Lp;
    ca.nlandmarks = nlandmarks;
    ca.obs_zx = pf->e->d_obs_zx;
    ca.obs_zy = pf->e->d_obs_zy;
    ca.meas_var = pf->cfg.meas_var;
    ca.live_in = pf->live[pf->live_cur];
    ca.live_out = pf->live[1 - pf->live_cur];
    ca.cnt = pf->cov_cnt;
    ca.phase = pf->cov_phase;
    ca.cstamp = pf->cstamp;
    ca.stamp_now = pf->cstamp_now;
    ca.h_live = dev_word(pf, RES_LIVE);
    ca.h_mark = dev_word(pf, RES_CLS_MARK);
    ca.epoch = pf->cls_epoch;
    ca.mark = pf->cls_appended;
    pf->live_cur = 1 - pf->live_cur;
    pf->cov_phase = (pf->cov_phase + 1) % 3;
}

// the classes' update of the frame + the weights: ONE launch
int weights_with_classes(slam_pf* pf, int nlandmarks, bool use_ekf, bool save_prior = false)
{
    CovArgs ca;
    int bound = 0;
    split_class_prepare(pf, nlandmarks, save_prior, ca, bound);
    return slam_logweight_cov_dev(pf->e, pf->score, use_ekf, pf->cfg.score_gain, pf->n, pf->logw, nullptr, &ca, bound);
}

// the particles' side of a split update: the classes follow their particles through it; it stamps the ones still in use
SplitIO split_io(const slam_pf* pf, int group_filter, const int32_t* map_anc)
{
    SplitIO sio{};
    sio.group_filter = group_filter;
    sio.map_anc = map_anc;
    sio.cov = pf->cov;
    sio.cov_stride = pf->cov_stride();
    sio.covx = pf->covx;
    sio.covx_stride = pf->mean_stride();
    sio.cls_in = pf->cls[pf->sp_cur];
    sio.cls_out = pf->cls[1 - pf->sp_cur];
    sio.cstamp = pf->cstamp;
    sio.stamp_now = pf->cstamp_now + 1;
    return sio;
}

FrameFacts frame_facts(const slam_pf* pf, int use_observations)
{
    FrameFacts f{};
    f.ekf = pf->L > 0 && use_observations;
    f.observing = f.ekf && pf->e->obs_nlandmarks == pf->L;
    // SLAM_MAP_AUTO samples the number of observed landmarks: every frame at the start and while the counts speak against
    // the current layout, every 8th frame otherwise
    f.sample_obs = pf->layout_cfg == SLAM_MAP_AUTO && !pf->auto_stuck && f.observing &&
                   (pf->frame < 8 || (pf->frame & 7u) == 0 || (pf->paged ? pf->votes_rows : pf->votes_pages) > 0);
    f.localise = pf->known_on && use_observations;
    f.anc = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    f.src = pf->pose[pf->cur];
    f.dst = pf->pose[1 - pf->cur];
    f.first_id = (int64_t)pf->rank * pf->n;
    f.count = pf->page_scratch + pool_state_words();
    f.tpage = f.count + 1;
    f.tindex = f.tpage + pf->nb;
    f.tmask = f.tindex + pf->nb;
    f.tbase = f.tmask + pf->nb;
    int32_t* lst = f.tbase + pf->nb + 1;
    if (pf->paged && pf->L <= kObsListMaxLandmarks)   // id[Lp] | zx[Lp] | zy[Lp] | round[Lp] | {count, highest round}
        f.lo = ObsListOut{ lst, reinterpret_cast<float*>(lst + pf->Lp), reinterpret_cast<float*>(lst + 2 * pf->Lp), lst + 3 * pf->Lp,
                           lst + 4 * pf->Lp };
    return f;
}

// the paged update into fresh pages; split pages: mean pages of two planes, the covariances per class
PagedEkfArgs paged_ekf_args(const slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    const size_t sn = (size_t)pf->n;
    PagedEkfArgs a;
    a.ol = ObsListView{ f.lo.id, f.lo.zx, f.lo.zy, f.lo.round, f.lo.count };
    a.tmask = f.tmask;
    a.tbase = f.tbase;
    a.pool = pf->pool;
    if (pf->split) {
        a.geom = split_geom(pf);
        a.pool = split_pool(pf);
        a.cov = pf->cov;
        a.covx = pf->covx;
        a.plane_stride = pf->Lp;
        a.cls_in = pf->cls[pf->sp_cur];
        a.cls_out = pf->cls[1 - pf->sp_cur];
        a.cstamp = pf->cstamp;
        a.cstamp_now = pf->cstamp_now + 1;
    }
    a.pt_in = pf->pt[pf->pt_cur];
    a.pt_out = pf->pt[1 - pf->pt_cur];
    a.nb = pf->nb;
    a.anc = f.anc;
    a.n = pf->n;
    a.nlandmarks = pf->L;
    a.x = f.dst;
    a.y = f.dst + sn;
    a.th = f.dst + 2 * sn;
    a.obs_zx = e->d_obs_zx;
    a.obs_zy = e->d_obs_zy;
    a.meas_var = pf->cfg.meas_var;
    a.loglik = e->ll_buf.as<float>();
    a.loglik_user = nullptr;
    a.tpage = f.tpage;
    a.tindex = f.tindex;
    a.count = f.count;
    a.freelist = pf->freelist;
    a.pool_state = pf->page_scratch;
    a.stamp = pf->stamp;
    a.stamp_now = pf->stamp_now + 1;   // the stamp of the tables this update writes
    return a;
}

// SLAM_MAP_AUTO's sample of the number of landmarks this frame observes, where no page list takes it along
int issue_obs_count(slam_pf* pf)
{
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, launch_obs_count(e->stream, e->d_obs_zx, e->d_obs_zy, pf->L, dev_word(pf, RES_OBS), ++pf->obs_seq_issued, pf->votes));
    return SLAM_OK;
}

// the weights of a frame whose landmark update left no log-likelihoods (no observations used)
int plain_weights(slam_pf* pf) { return slam_logweight_dev(pf->e, pf->score, nullptr, pf->cfg.score_gain, pf->n, pf->logw, nullptr); }

// Paged maps: the frame's page list (touched pages, observation list, where the fresh pages come from)
int issue_page_list(slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    const ProfScope prof(e, SLAM_PROF_PAGES);
    SLAM_HIP_TRY(e, launch_page_list(e->stream, e->d_obs_zx, e->d_obs_zy, pf->L, pf->nb, f.tpage, f.tindex, f.tmask, f.tbase, f.count, pf->n,
                                     pf->page_scratch, f.sample_obs ? dev_word(pf, RES_OBS) : nullptr, f.sample_obs ? ++pf->obs_seq_issued : 0,
                                     f.sample_obs ? pf->votes : nullptr, dev_word(pf, RES_PAGE_HINT), f.lo));
    return SLAM_OK;
}

// a new free list when the old one runs short (decided on the device; the pages in use carry the last stamp)
int issue_free_list(slam_pf* pf)
{
    SLAM_HIP_TRY(pf->e, launch_free_list(pf->e->stream, pf->stamp, pf->npages, pf->stamp_now, pf->freelist, pf->page_scratch,
                                         dev_word(pf, RES_SHORT_LIST)));
    return SLAM_OK;
}

// 1 + 2. motion (+ the fused gather of the previous resample) and scan-match score, one launch.  Sharded: the ancestors' poses come
// out of the array of every rank's poses: it needs nothing from the exchange and keeps the GPU busy while the host picks up the plan.
int front_stage(slam_pf* pf, FrameFacts& f, int slot, const float dp[3])
{
    slam_engine* e = pf->e;
    slam_comm* comm = pf->comm;
    const int n = pf->n;
    const size_t sn = (size_t)n;
    float* dst = f.dst;
    // Where the ancestors' poses are.  (Sharded: the wait for their all-gather.  Nothing of a sharded frame is issued between here
    // and its front launch: the page list below and the survivor rows are for one GPU.)
    const float* ps = nullptr;
    const int32_t* pose_anc = nullptr;
    if (int rc = ancestor_poses(pf, &ps, &pose_anc)) return rc;
    // Paged maps on one GPU: the page list goes out first and the free list it may ask for travels in workgroups of the scorer's
    // launch (free_list_body.h).  A sharded session issues both behind its exchange, which takes pages from the same list first.
    FreeListRider rider;
    if (!comm && pf->paged && f.observing) {
        if (int rc = issue_page_list(pf, f)) return rc;
        rider = FreeListRider{ pf->stamp, pf->npages, pf->stamp_now, pf->freelist, pf->page_scratch, dev_word(pf, RES_SHORT_LIST) };
        f.paged_listed = true;
    }
    // Survivor rows: the switch is on, the frame goes to the fused front launch and the session has (or now gets) the buffers;
    // whether the launch takes the frame is known for good once it has been asked.  A frame that cannot be one reads,
    // gathers or overwrites whole mean buffers: the rows the frame before left unwritten come first.
    const bool want_survivors = e->survivor_rows && pf->split && !pf->paged && !comm && pf->refine_sweeps == 0 && f.anc &&
                                f.observing && e->frame_fusion && !(e->prof_mask & (1 << SLAM_PROF_SCORE)) &&
                                frame_front_fits(pf->n, pf->L, 4) && survivor_buffers(pf);
    if (!want_survivors)
        if (int rc = settle_means(pf)) return rc;
    // 1 + 2 + 3 in ONE launch when the frame allows it (landmarks observed, long rows, enough particles): motion + score and the
    // out-of-place landmark update side by side (slam_frame_front_dev; the same bits).  One GPU, rows or split: a gated session
    // on rows is left out (its frames that keep their population update in place; on split they go through the identity index).
    // Sharded, split, ungated: the launch scores every particle (poses out of the all-gathered array) and updates the groups
    // whose ancestors are all rows of this rank; the groups with an ancestor in the staging tail follow behind the exchange
    // (update_split).  Like the motion + score launch it replaces, it goes out before the host has looked at the plan.
    // Refining session: motion + refine, the frame as it runs while SLAM_PROF_SCORE is timed — no fused front (its update would
    // work out the UNREFINED sample again): the update stages read the refined poses from dst.
    if (pf->refine_sweeps > 0) {
        if (int rc = slam_motion_refine_dev(e, slot, ps, ps + sn, ps + 2 * sn, pose_anc, dst, dst + sn, dst + 2 * sn, n, f.first_id, dp,
                                            pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->refine_step_xy, pf->refine_step_theta,
                                            pf->refine_sweeps, pf->score, pf->count))
            return rc;
        if (f.paged_listed) {
            const ProfScope prof(e, SLAM_PROF_PAGES);
            return issue_free_list(pf);
        }
        return SLAM_OK;
    }
    // General measurement covariance (rows only): its update exists as a launch of its own alone.
    // Data association likewise: associate + update, two launches that read the poses this one writes.
    const bool front = !pf->aniso && !pf->assoc_on && (comm ? pf->split && !pf->paged && pf->has_anc && !pf->gated : !pf->paged && (!pf->gated || pf->split));
    if (front && f.anc && f.observing) {
        const SplitIO sio = pf->split ? split_io(pf, comm ? 1 : 0, comm ? f.anc : nullptr) : SplitIO{};
        const float* map_in = pf->split ? pf->mean[pf->sp_cur] : pf->map[pf->map_cur];
        float* map_out = pf->split ? pf->mean[1 - pf->sp_cur] : pf->map[1 - pf->map_cur];
        // (a survivor-rows frame may come back with its weights made as well: one workgroup scores and updates a particle)
        const slam_front_weights fw{ pf->cfg.score_gain, pf->logw, &f.weighted };
        if (int rc = slam_frame_front_dev(e, slot, ps, ps + sn, ps + 2 * sn, pose_anc, dst, dst + sn, dst + 2 * sn, n, f.first_id, dp,
                                          pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->score, pf->count, map_in, map_out,
                                          pf->split ? pf->mean_stride() : pf->row_stride(), pf->Lp, pf->L, pf->cfg.meas_var, &f.fused,
                                          pf->split ? &sio : nullptr, want_survivors ? pf->obs_save : nullptr,
                                          want_survivors ? &fw : nullptr))
            return rc;
        f.survivors = f.fused && want_survivors;
        if (f.survivors) {   // (the rows of the frame before are read through its gather index only: no settle)  What this frame starts from:
            pf->surv.mean_in = map_in;
            pf->surv.mean_out = map_out;
            pf->surv.anc = f.anc;
            pf->surv.cls_in = sio.cls_in;
            pf->surv.pose = dst;
            int32_t info[2];
            if (int rc = slam_frame_front_last(e, info)) return rc;
            pf->surv.group = info[0];
            pf->surv.pending = false;   // (its own rows become pending behind the resample)
        }
    }
    if (f.survivors) return SLAM_OK;
    if (int rc = settle_means(pf)) return rc;   // (the launch did not take the shapes: nothing was issued yet)
    if (f.fused) return SLAM_OK;
    if (comm && pf->has_anc)
        return slam_motion_score_dev(e, slot, ps, ps + sn, ps + 2 * sn, pose_anc, dst, dst + sn, dst + 2 * sn, n, f.first_id, dp,
                                     pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->score, pf->count);
    bool rode = false;
    if (int rc = slam_motion_score_rider_dev(e, slot, ps, ps + sn, ps + 2 * sn, pose_anc, dst, dst + sn, dst + 2 * sn, n, f.first_id,
                                             dp, pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->score, pf->count,
                                             f.paged_listed ? &rider : nullptr, &rode))
        return rc;
    if (f.paged_listed && !rode) {   // (a small population: its scorer has no room for a rider)
        const ProfScope prof(e, SLAM_PROF_PAGES);
        return issue_free_list(pf);
    }
    return SLAM_OK;
}

// Resample gate: did the previous frame keep its population?  (Its verdict was made on the device; the host looks at it
// only now, behind the front launch — a flag in mapped memory.)  Then the maps have not moved: on rows the EKF runs IN PLACE.
// Sharded: then map rows of remote ancestors -> staging tail; issued behind the front launch, which does not need them.
int gate_and_exchange(slam_pf* pf, FrameFacts& f, bool* collective_verdict)
{
    if (pf->gated && pf->has_anc) {
        int resampled = 1;
        if (int rc = slam_resample_happened_host(pf->e, &resampled)) return rc;
        f.in_place = !resampled;
        pf->frames_resampled += resampled ? 1 : 0;
    }
    if (pf->comm)
        if (int rc = finish_exchange(pf)) {
            *collective_verdict = rc == SLAM_ERR_CAPACITY;
            return rc;
        }
    return SLAM_OK;
}

// which measurement noise this frame's landmark update (and its association) uses on rows: the 2x2 covariance in force — the
// association's own while association is on (slam_pf_assoc_cov_set), else slam_pf_meas_cov_set's — or meas_var * I
slam_meas_noise update_noise(const slam_pf* pf)
{
    if (pf->assoc_on && pf->assoc_detcov) return slam_meas_noise{ 0.0f, nullptr, false, true };   // the detections' own Q_k
    if (pf->assoc_on ? pf->assoc_aniso : pf->aniso) return slam_meas_noise{ 0.0f, pf->assoc_on ? pf->assoc_cov : pf->meas_cov, true };
    return slam_meas_noise{ pf->cfg.meas_var, nullptr, false };
}


// 3. per-landmark EKF (+ fused gather) and the weights, one function per storage form.  Rows: in place, out of place, gather only
int update_rows(slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    const int n = pf->n, L = pf->L, mc = pf->map_cur, mn = 1 - mc;
    const size_t sn = (size_t)n;
    const int64_t stride = pf->row_stride();
    float* dst = f.dst;
    if (f.localise) {   // a known map (no maps of the session's own): the stage on the poses the front launch left, the clutter term, the weights
        // (the map as it was given lies behind the prepared one)
        if (pf->known_miss_on) {   // the miss form of either stage: behind the table of this frame's scan where line of sight is on
            if (pf->known_sight_bins)
                if (int rc = slam_sight_table_dev(e, pf->known_sight_bins)) return rc;
            int32_t* cnt = pf->known_missed;
            if (int rc = (pf->known_detcov ? slam_localise_detcov_miss_dev : slam_localise_miss_dev)(
                    e, pf->known_detcov ? pf->known_prep + 6 * (size_t)pf->known_Lp : pf->known_prep, pf->known_Lp, pf->known_L, dst, dst + sn,
                    dst + 2 * sn, n, pf->known_gate, nullptr, 0, pf->known_stats, nullptr, &pf->known_view, cnt, cnt + sn, cnt + 2 * sn))
                return rc;
            pf->known_ll = true;
            if (pf->known_log_clutter != 0.0f || pf->known_log_miss != 0.0f)
                if (int rc = slam_assoc_weight_dev(e, pf->known_stats, cnt, n, 0.0f, pf->known_log_clutter, pf->known_log_miss, nullptr, nullptr))
                    return rc;
            return slam_logweight_ekf_dev(e, pf->score, pf->cfg.score_gain, n, pf->logw, nullptr);
        }
        if (int rc = pf->known_detcov ? slam_localise_detcov_dev(e, pf->known_prep + 6 * (size_t)pf->known_Lp, pf->known_Lp, pf->known_L, dst, dst + sn,
                                                                 dst + 2 * sn, n, pf->known_gate, nullptr, 0, pf->known_stats, nullptr)
                                      : slam_localise_dev(e, pf->known_prep, pf->known_Lp, pf->known_L, dst, dst + sn, dst + 2 * sn, n, pf->known_gate,
                                                          nullptr, 0, pf->known_stats, nullptr))
            return rc;
        pf->known_ll = true;
        if (pf->known_log_clutter != 0.0f)
            if (int rc = slam_assoc_weight_dev(e, pf->known_stats, nullptr, n, 0.0f, pf->known_log_clutter, 0.0f, nullptr, nullptr)) return rc;
        return slam_logweight_ekf_dev(e, pf->score, pf->cfg.score_gain, n, pf->logw, nullptr);
    }
    if (f.ekf) {
        if (f.sample_obs)
            if (int rc = issue_obs_count(pf)) return rc;
        // (fused: the update went out with the score; in place: no gather, the buffers do not flip)
        float* out = pf->map[f.in_place ? mc : mn];
        const int32_t* anc = f.in_place ? nullptr : f.anc;
        const slam_meas_noise noise = update_noise(pf);
        if (pf->assoc_on) {   // detections without identity: the observation table is not read
            const slam_assoc_view table{ pf->assoc_tab, pf->Lp };
            if (int rc = slam_engine_associate(e, pf->map[mc], stride, pf->Lp, L, dst, dst + sn, dst + 2 * sn, anc, n, noise, pf->assoc_gate,
                                               pf->assoc_new_gate, pf->assoc_create, pf->assoc_tab, pf->Lp, pf->assoc_stats))
                return rc;
            if (int rc = slam_engine_ekf_update(e, pf->map[mc], out, stride, pf->Lp, L, dst, dst + sn, dst + 2 * sn, anc, n, noise, &table, nullptr))
                return rc;
            // existence evidence, on the row the update wrote: through the frame's gather into the other buffer, or in place
            int32_t* missed = pf->assoc_weight_on ? pf->assoc_weight_missed : nullptr;   // the stage's misses, for the weight below
            if (pf->prune_on) {   // ... in the form that is switched on; line of sight: the table of this frame's scan first
                if (pf->sight_bins)
                    if (int rc = slam_sight_table_dev(e, pf->sight_bins)) return rc;
                const slam_evidence_form form{ dst + 2 * sn, pf->sight_margin, pf->sight_bins != 0, pf->fov_on, pf->fov_lo, pf->fov_hi,
                                               pf->sight_spared, pf->fov_outside };
                if (int rc = slam_engine_evidence(e, out, stride, pf->Lp, L, dst, dst + sn, anc, n, pf->assoc_tab, pf->Lp, pf->ev[mc],
                                                  pf->ev[f.in_place ? mc : mn], pf->Lp, pf->prune_hit, pf->prune_miss, pf->prune_cmax,
                                                  pf->prune_range, pf->ev_stats, missed, form))
                    return rc;
            }
            // duplicates: behind the update and the evidence stage, in place on the row and the evidence buffer this frame wrote
            if (pf->merge_gate != 0.0f)
                if (int rc = slam_landmark_merge_dev(e, out, stride, pf->Lp, L, n, pf->assoc_tab, pf->Lp,
                                                     pf->prune_on ? pf->ev[f.in_place ? mc : mn] : nullptr, pf->Lp, pf->prune_cmax,
                                                     pf->merge_gate, pf->merge_stats))
                    return rc;
            // the unexplained: created, dropped and missed enter the log-likelihood the update left, in front of the weights
            if (pf->assoc_weight_on)
                if (int rc = slam_assoc_weight_dev(e, pf->assoc_stats, pf->prune_on ? missed : nullptr, n, pf->assoc_weight_log[0],
                                                   pf->assoc_weight_log[1], pf->assoc_weight_log[2], nullptr, pf->assoc_weight_terms))
                    return rc;
        } else if (!f.fused) {
            if (int rc = slam_engine_ekf_update(e, pf->map[mc], out, stride, pf->Lp, L, dst, dst + sn, dst + 2 * sn, anc, n, noise, nullptr, nullptr))
                return rc;
        }
        if (!f.in_place) pf->map_cur = mn;
        return slam_logweight_ekf_dev(e, pf->score, pf->cfg.score_gain, n, pf->logw, nullptr);
    }
    if (L > 0 && f.anc && !f.in_place) {   // the maps follow their particles even without an observation
        if (int rc = slam_gather_map_dev(e, pf->map[mc], pf->map[mn], stride, stride, pf->Lp, pf->Lp, L, f.anc, n)) return rc;
        if (pf->prune_on)   // ... and so does their evidence
            if (int rc = slam_evidence_gather_dev(e, pf->ev[mc], pf->ev[mn], pf->Lp, f.anc, n)) return rc;
        pf->map_cur = mn;
    }
    return plain_weights(pf);
}

int update_split(slam_pf* pf, FrameFacts& f)
{
    slam_engine* e = pf->e;
    const int n = pf->n, L = pf->L, sc = pf->sp_cur;
    const size_t sn = (size_t)n;
    float* dst = f.dst;
    if (f.ekf) {
        if (!f.observing) return SLAM_ERR_NOT_READY;
        if (f.sample_obs)
            if (int rc = issue_obs_count(pf)) return rc;
        // the particles' update (a frame that kept its population: out of place all the same, through the identity index); behind
        // a sharded fused front: the groups that waited for the exchange — no rows received: the launch would find nothing to do ...
        if (!f.fused || (pf->comm && pf->rows_received > 0)) {
            const SplitIO sio = split_io(pf, f.fused ? 2 : 0, nullptr);
            if (int rc = slam_ekf_split_dev(e, pf->mean[sc], pf->mean[1 - sc], pf->mean_stride(), pf->Lp, L, dst, dst + sn, dst + 2 * sn,
                                            f.anc, n, pf->cfg.meas_var, &sio))
                return rc;
        }
        pf->cstamp_now++;
        pf->sp_cur = 1 - sc;
        // ... then the classes' update, in place, once per class still in use: with the weights — or, when the front launch has
        // made those, with the scan (scan_stage): it still runs behind the launch that stamped the classes and in front of the
        // one that reads the saved priors
        if (f.weighted) {
            split_class_prepare(pf, L, f.survivors, f.cov, f.cov_bound);
            f.classes_due = true;
            return SLAM_OK;
        }
        return weights_with_classes(pf, L, true, f.survivors);
    }
    if (f.anc) {   // means and classes follow their particles
        const ProfScope prof(e, SLAM_PROF_PAGES);
        SLAM_HIP_TRY(e, launch_split_gather(e->stream, pf->mean[sc], pf->mean[1 - sc], pf->cls[sc], pf->cls[1 - sc], pf->Lp, f.anc, n,
                                            pf->cstamp, ++pf->cstamp_now));
        pf->sp_cur = 1 - sc;
        return weights_with_classes(pf, 0, false);   // no observations: the list of classes in use only
    }
    return plain_weights(pf);
}

// pages and split pages: touched pages of this frame's observation table, the update into fresh pages, the next free list
int update_paged(slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    const int n = pf->n, pc = pf->pt_cur;
    if (f.ekf) {
        if (!f.observing) return SLAM_ERR_NOT_READY;
        SLAM_HIP_TRY(e, e->ll_buf.ensure(sizeof(float) * (size_t)n));
        if (!f.paged_listed) {
            if (int rc = issue_page_list(pf, f)) return rc;
            const ProfScope prof(e, SLAM_PROF_PAGES);
            if (int rc = issue_free_list(pf)) return rc;
        }
        const PagedEkfArgs a = paged_ekf_args(pf, f);
        pf->stamp_now++;
        // pages staged per pass = what the last frames touched (a hint in mapped memory, read without waiting)
        SLAM_HIP_TRY(e, launch_ekf_paged(e->stream, a, e->prof_next(SLAM_PROF_EKF), f.lo.id ? 1 : 0,
                                         __atomic_load_n(host_word(pf, RES_PAGE_HINT), __ATOMIC_RELAXED)));
        e->ll_n = n;
        pf->pt_cur = 1 - pc;
        if (!pf->split) return slam_logweight_ekf_dev(e, pf->score, pf->cfg.score_gain, n, pf->logw, nullptr);
        // the classes went with their particles; their covariances, once per class, with the weights
        pf->cstamp_now++;
        pf->sp_cur = 1 - pf->sp_cur;
        return weights_with_classes(pf, pf->L, true);
    }
    if (!f.anc) return plain_weights(pf);
    {   // the tables follow their particles ...
        const ProfScope prof(e, SLAM_PROF_PAGES);
        SLAM_HIP_TRY(e, launch_page_table_gather(e->stream, pf->pt[pc], pf->pt[1 - pc], pf->nb, f.anc, n, pf->stamp, ++pf->stamp_now));
        pf->pt_cur = 1 - pc;
        if (pf->split) {   // ... and so do the classes
            SLAM_HIP_TRY(e, launch_class_gather(e->stream, pf->cls[pf->sp_cur], pf->cls[1 - pf->sp_cur], f.anc, n, pf->cstamp,
                                                ++pf->cstamp_now));
            pf->sp_cur = 1 - pf->sp_cur;
        }
    }
    return pf->split ? weights_with_classes(pf, 0, false) : plain_weights(pf);
}

// 4. weights: the maximum over all ranks, then fixed-point weights scanned as they are produced (a frame whose front launch made
// the weights: the scan's launch carries the classes' update that the weights' launch would have carried)
// Sharded: the ranks all-reduce the BLOCK maxima the weights' launch leaves in the engine (element by element: a few hundred
// floats cost the wire what one costs) and the scan takes their maximum itself, as it does on one GPU — the maximum of the
// same set of values, and one single-workgroup launch less per frame than reducing them to one float first.
int scan_stage(slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    if (f.classes_due) return slam_quantise_scan_cov_dev(e, pf->logw, pf->n, &f.cov, f.cov_bound);   // (one GPU, no gate)
    if (pf->comm) {
        if (e->bmax_n != pf->n || e->bmax_count <= 0) return SLAM_ERR_NOT_READY;
        if (int rc = comm_all_reduce_max_f32(pf->comm, e->bmax_buf.as<float>(), e->bmax_count)) return rc;
    }
    return slam_quantise_scan_dev(e, pf->logw, nullptr, pf->n, pf->comm ? pf->d_sum : nullptr);
}

// 5. resample on the integer CDF
int resample_stage(slam_pf* pf, const float* poses, bool survivors)
{
    slam_engine* e = pf->e;
    slam_comm* comm = pf->comm;
    const int n = pf->n, nxt = 1 - pf->cur;
    const size_t sn = (size_t)n;
    if (survivors) {   // one GPU: the search also marks the particles it keeps, and one launch behind it writes their mean rows
        const SurvivorOut so{ pf->survivor, ++pf->surv_stamp };
        if (int rc = slam_ancestors_survivors_dev(e, n, pf->cfg.seed, pf->frame, pf->anc[nxt], &so)) return rc;
        pf->surv.pending = true;
        return materialise(pf, true);
    }
    if (!comm) return slam_ancestors_from_scan_dev(e, n, pf->cfg.seed, pf->frame, pf->anc[nxt]);
    // shard totals (with the gate: total, sum v, sum v^2 per rank)
    if (int rc = comm_all_gather(comm, pf->d_sum, pf->totals, (pf->gated ? 3 : 1) * sizeof(uint64_t))) return rc;
    if (int rc = slam_offspring_from_scan_sharded_dev(e, n, pf->totals, pf->rank, pf->world, pf->cfg.seed, pf->frame, pf->n_total,
                                                      pf->first))
        return rc;
    // the "all-gather of surviving indices" (4 B x N_total) and, grouped into the same RCCL launch, this frame's poses
    // to every rank (12 B x N_total) for the next frame's motion + score — that launch then needs nothing from the exchange
    if (int rc = comm_all_gather2(comm, pf->first, pf->first_all, sn * sizeof(int32_t), poses, pf->pose_all, 3 * sn * sizeof(float)))
        return rc;
    // 6. gather index of every slot (remote ancestors -> rows of the staging tail) and the exchange plan, on the
    // device; the exchange itself happens at the start of the next frame, behind its motion + score launch
    if (int rc = slam_ancestors_sharded_dev(e, pf->first_all, pf->n_total, n, pf->rank, pf->world, pf->anc[nxt], pf->d_plan,
                                            pf->pose_idx[nxt]))
        return rc;
    pf->exchange_pending = true;
    return SLAM_OK;
}

// Map rows (and poses) of ancestors that live on another rank -> the staging tail of the current buffers, where
// the next EKF's fused gather picks them up.  pack (one launch) -> one grouped send/recv -> unpack (one launch).
// A remote ancestor travels once per destination rank, however many slots there descend from it.
int migrate(slam_pf* pf)
{
    slam_engine* e = pf->e;
    const int G = pf->world, n = pf->n, L = pf->L;
    int32_t plan[SLAM_PLAN_WORDS(kMaxRanks)];
    // the one point of a frame where the host waits for the device (a flag in mapped memory, no copy, no stream sync)
    if (int rc = slam_exchange_plan_host(e, G, plan)) return rc;
    if (plan[0] & 2) {   // the same verdict on every rank: all refuse the frame together
        snprintf(e->err, sizeof e->err, "exchange might exceed recv_capacity %d on some rank", pf->recv_cap);
        return SLAM_ERR_CAPACITY;
    }
    pf->rows_received = 0;
    if (!(plan[0] & 1) && G > 1) return SLAM_OK;   // every run boundary coincides with a rank boundary: all ranks skip
    const int32_t *scnt = plan + 1, *rcnt = plan + 1 + G;
    int64_t stot = 0, rtot = 0, sfl[kMaxRanks], rfl[kMaxRanks];
    const int64_t rec = 3 + 5 * (int64_t)L;
    for (int q = 0; q < G; ++q) {
        stot += scnt[q];
        rtot += rcnt[q];
        sfl[q] = rec * scnt[q];
        rfl[q] = rec * rcnt[q];
    }
    if (rtot > pf->recv_cap) return SLAM_ERR_CAPACITY;   // cannot happen: bit 1 above bounds it
    pf->rows_received = (int)rtot;
    if (int rc = grow(pf, &pf->sbuf, &pf->sbuf_floats, (size_t)(rec * stot))) return rc;
    if (int rc = grow(pf, &pf->rbuf, &pf->rbuf_floats, (size_t)(rec * rtot))) return rc;
    const bool split = L && pf->split, spages = split && pf->paged;   // (split pages: the means on pages of two planes, the classes as on split)
    const PageGeom geom = spages ? split_geom(pf) : PageGeom();
    const float* mp = L ? (spages ? split_pool(pf) : pf->paged ? pf->pool : split ? pf->mean[pf->sp_cur] : pf->map[pf->map_cur]) : nullptr;
    if (stot)
        if (int rc = slam_migrate_pack_paged(e, n, pf->rank, G, plan, pf->pose[pf->cur], n, mp, split ? pf->mean_stride() : pf->row_stride(),
                                             pf->Lp, L, pf->sbuf, pf->paged ? pf->pt[pf->pt_cur] : nullptr, pf->nb, split ? pf->cov : nullptr,
                                             split ? pf->cls[pf->sp_cur] : nullptr, spages ? &geom : nullptr))
            return rc;
    if (int rc = comm_all_to_all_f32(pf->comm, pf->sbuf, sfl, pf->rbuf, rfl)) return rc;
    if (rtot && (split || pf->paged)) {
        const ProfScope prof(e, SLAM_PROF_UNPACK);
        if (split) {
            // every received row becomes a class of its own (it brings its covariances along); its number comes from the free list
            // of classes on the device, made anew from the stamps when its guaranteed length — a rank's staging rows: at most n
            // classes are in use — is used up (SLAM_SPLIT_CLASS_ROOM: tests make the lists short)
            const char* room_env = getenv("SLAM_SPLIT_CLASS_ROOM");
            const int64_t room = room_env && atoi(room_env) > 0 && atoi(room_env) < pf->recv_cap ? atoi(room_env) : pf->recv_cap;
            if (pf->cls_cursor + rtot > room) {
                SLAM_HIP_TRY(e, launch_class_free_list(e->stream, pf->cstamp, pf->cap, pf->cstamp_now, pf->cls_free, pf->cls_fs));
                pf->cls_cursor = 0;
            }
        }
        if (pf->paged) {   // fresh pages for the received rows (a new free list first if the old one runs short), table rows n .. n + rtot - 1
            SLAM_HIP_TRY(e, launch_pool_reserve(e->stream, pf->page_scratch, rtot * pf->nb));
            if (int rc = issue_free_list(pf)) return rc;
        }
        if (spages)   // the means onto the fresh pages
            SLAM_HIP_TRY(e, launch_migrate_unpack_split_pages(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, page_pool(pf),
                                                              class_store(pf), L, pf->cfg.meas_var, pf->cls_free, (int)pf->cls_cursor));
        else if (split)
            SLAM_HIP_TRY(e, launch_migrate_unpack_split(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, pf->mean[pf->sp_cur],
                                                        class_store(pf), L, pf->cfg.meas_var, pf->cls_free, (int)pf->cls_cursor));
        else
            SLAM_HIP_TRY(e, launch_migrate_unpack_paged(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, page_pool(pf), L));
        if (split) {
            pf->cls_cursor += rtot;
            pf->cls_appended += (uint32_t)rtot;
        }
    } else if (rtot) {
        if (int rc = slam_migrate_unpack_dev(e, pf->rbuf, G, rcnt, n, pf->pose_stage, pf->cap,
                                             L ? pf->map[pf->map_cur] : nullptr, pf->row_stride(), pf->Lp, L))
            return rc;
    }
    return SLAM_OK;
}

int pf_step_impl(slam_pf* pf, int slot, const float dp[3], int use_observations, bool* collective_verdict)
{
    slam_engine* e = pf->e;
    if (pf->paged && __atomic_load_n(host_word(pf, RES_SHORT_LIST), __ATOMIC_ACQUIRE) != 0) {
        snprintf(e->err, sizeof e->err, "paged maps: a free list was shorter than the pages reserved from it (pool invariant broken)");
        return SLAM_ERR_CAPACITY;
    }
    if (int rc = auto_layout(pf)) return rc;   // may move the maps to another layout (never changes a result)
    FrameFacts f = frame_facts(pf, use_observations);
    // per-detection noise: an observing frame whose detections will carry no covariance (none uploaded and no detector; or the
    // session's detector has no noise model) is refused here, before its first launch — the session is as if the frame was never
    // asked for
    if (pf->assoc_on && pf->assoc_detcov && f.ekf && (pf->detect_on ? !pf->detect_noise_on : !e->det_has_cov)) {
        snprintf(e->err, sizeof e->err, "association under per-detection covariances (slam_pf_assoc_detcov_set): the frame's detections "
                                        "carry none (slam_detections_cov_upload_host / _set_dev, or slam_pf_detect_noise_set)");
        return SLAM_ERR_NOT_READY;
    }
    if (pf->known_detcov && f.localise && (pf->detect_on ? !pf->detect_noise_on : !e->det_has_cov)) {   // ... and the same for a known map
        snprintf(e->err, sizeof e->err, "localisation under per-detection covariances (slam_pf_known_map_detcov_set): the frame's detections "
                                        "carry none (slam_detections_cov_upload_host / _set_dev, or slam_pf_detect_noise_set)");
        return SLAM_ERR_NOT_READY;
    }
    // the detector: in front of the frame's first launch, so that its count has arrived when update_rows' association (or its
    // localise stage: a known map) asks for it
    if (pf->detect_on && (pf->assoc_on ? f.ekf : f.localise))
        if (int rc = slam_detect_scan_noise_dev(e, &pf->detect_params, pf->detect_fit_on ? &pf->detect_fit : nullptr,
                                                pf->detect_noise_on ? &pf->detect_noise : nullptr, nullptr))
            return rc;
    if (int rc = front_stage(pf, f, slot, dp)) return rc;
    if (int rc = gate_and_exchange(pf, f, collective_verdict)) return rc;
    if (int rc = pf->paged ? update_paged(pf, f) : pf->split ? update_split(pf, f) : update_rows(pf, f)) return rc;
    if (int rc = scan_stage(pf, f)) return rc;
    if (int rc = resample_stage(pf, f.dst, f.survivors)) return rc;
    pf->cur = 1 - pf->cur;
    pf->has_anc = true;
    pf->last_ekf = f.ekf || f.localise;
    pf->reseeded = false;   // (slam_pf_known_map_reseed: the log-weights are this frame's again)
    pf->frame++;
    return SLAM_OK;
}

}  // namespace

// ---- what the read-backs share with the frame
// Where the ancestors' poses are: pose[cur] behind the pending gather index (none: as they are); sharded with a gather pending:
// the array of every rank's poses, once its all-gather has arrived, behind the positions of the ancestors in it.
int ancestor_poses(slam_pf* pf, const float** base, const int32_t** idx)
{
    *base = pf->pose[pf->cur];
    *idx = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    if (!pf->comm || !pf->has_anc) return SLAM_OK;
    *base = pf->pose_all;
    *idx = pf->pose_idx[pf->cur];
    return comm_all_gather_finish(pf->comm);
}

int finish_exchange(slam_pf* pf)
{
    if (!pf->exchange_pending) return SLAM_OK;
    pf->exchange_pending = false;
    return migrate(pf);
}

}  // namespace slam::session

using namespace slam;
using namespace slam::session;

extern "C" {
int slam_pf_step(slam_pf* pf, int slot, const float dp[3], int use_observations)
{
    if (!pf || !dp) return SLAM_ERR_INVALID_ARG;
    bool collective_verdict = false;
    const int rc = pf_step_impl(pf, slot, dp, use_observations, &collective_verdict);
    // A frame that fails on THIS rank alone leaves the other ranks inside (or on their way into) a collective: give up
    // for good so that they get SLAM_ERR_COMM instead of waiting for ever.  A refusal every rank reaches together (the
    // staging area might overflow: bit 1 of the plan) is not such a failure.
    if (rc != SLAM_OK && pf->comm && !collective_verdict) (void)comm_abort(pf->comm);
    return rc;
}
}  // extern "C"
