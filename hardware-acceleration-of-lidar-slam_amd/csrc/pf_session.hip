// pf_session.hip — the slam_pf_* session of include/slam_hip.h: device buffers + one whole frame per call, for a
// plain C host.  One GPU (slam_pf_create) or one rank of a population sharded over several GPUs
// (slam_pf_create_sharded): the frame is built on the public stage entry points either way, and in the sharded
// form every exchange step between the ranks is issued from here through comm.h (RCCL over xGMI, or the
// in-process transport) — nothing but this file sits between the launches.
// The landmark maps are kept as rows, pages, split (means per particle, covariances per class) or split pages; a
// SLAM_MAP_AUTO session lives on split and moves its means onto pages and back while it runs (auto_layout).
// No counterpart in the reference; specification: oracle/slam_oracle_pf.c; the shape
// "handle created once in main and threaded through" is the reference's (Hadrware_acclereated.cpp:842-845, 284).

#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>
#include <vector>

#include "comm.h"
#include "engine_internal.h"
#include "kernels.h"

using namespace slam;

// The 32 words of the engine's mapped result block (slam_pf::h_res as the host sees it, d_hres as the device does)
enum ResWord {
    RES_PAYLOAD = 0,      // 0..15: 8 x 8 bytes, what slam_pf_best / slam_pf_mean ask for
    RES_SEQ = 16,         // the sequence number behind the payload
    RES_CLS_MARK = 18,    // 18..19 {classes appended as of the last classes' update, its epoch} (cov_update_body.h)
    RES_SHORT_LIST = 20,  // "a free list came out shorter than its reservation" (paged maps; see free_list_kernel)
    RES_LIVE = 22,        // 22..23 {classes in use, epoch}
    RES_OBS = 24,         // 24..28 SLAM_MAP_AUTO's sample {observed, L, seq, votes_pages, votes_rows}, left by
    RES_OBS_SEQ = 26,     //        page_list_kernel / obs_count_kernel
    RES_VOTES_PAGES = 27, RES_VOTES_ROWS = 28,
    RES_PAGE_HINT = 30,   // pages the last frames touched per pass (page_list_kernel)
};

struct slam_pf {
    slam_engine* e = nullptr;
    slam_pf_config cfg{};
    int n = 0, L = 0;
    float* pose[2] = { nullptr, nullptr };     // [3][n] each
    float* map[2] = { nullptr, nullptr };      // [cap][5][Lp] each: one row per particle, planes padded to Lp floats
    int Lp = 0;                                // plane stride: L rounded up to 32 floats (128-byte rows)
    int32_t* anc[2] = { nullptr, nullptr };
    float *score = nullptr, *logw = nullptr;
    int32_t *count = nullptr, *first = nullptr;
    int cur = 0;       // pose / ancestor buffer holding the current particles
    int map_cur = 0;   // map buffer holding the current maps (flips only when the maps are rewritten)
    bool has_anc = false;
    uint32_t frame = 0;

    // ---- sharded form (comm != nullptr): this rank holds particles [rank*n, (rank+1)*n) of world*n
    slam_comm* comm = nullptr;
    int rank = 0, world = 1, recv_cap = 0, cap = 0;   // cap = n + recv_cap rows per map buffer (staging tail)
    int64_t n_total = 0;
    float* pose_all = nullptr;      // [world][x|y|theta][n]: every rank's poses, all-gathered each frame beside the EKF
    float* pose_stage = nullptr;    // [3][cap]: where the poses inside migrated records land (nothing reads them)
    int32_t* pose_idx[2] = { nullptr, nullptr };   // position of every slot's ancestor in pose_all
    int32_t* first_all = nullptr;   // [n_total]
    uint64_t *d_sum = nullptr, *totals = nullptr;   // shard total; all-gathered shard totals [world]
    int32_t* d_plan = nullptr;      // exchange plan of the frame, device copy
    float *sbuf = nullptr, *rbuf = nullptr;   // grow-only exchange buffers
    size_t sbuf_floats = 0, rbuf_floats = 0;
    bool exchange_pending = false;  // resample done, map rows not exchanged yet
    int rows_received = 0;
    // results a host asks for every frame (heaviest particle, posterior mean): written by ONE kernel to mapped host
    // memory behind a sequence number — no device-to-host copies, no stream synchronisation
    float* h_res = nullptr;         // pinned + mapped: the words of ResWord
    float* d_hres = nullptr;        // the same memory as the device sees it
    uint32_t res_seq = 0;
    float* res_dev = nullptr;       // device copy of the payload (what the ranks all-gather)
    unsigned long long* sums_acc = nullptr;   // 9 accumulators + ticket of pose_sums_kernel (kept zeroed by the kernel)
    void* res_all = nullptr;        // [world] payloads
    // ---- paged maps (slam_pf_paged_set before the session is made; one GPU): copy-on-write pages behind a page table
    // per particle instead of one row per particle (paged_kernels.hip); map[] stays unallocated
    bool paged = false;
    int nb = 0, npages = 0;         // pages per particle; pages in the pool (2 * cap * nb: never fewer than half are free)
    float* store = nullptr;         // the one allocation behind map[0], map[1] and pool
    int32_t* votes = nullptr;       // [2] SLAM_MAP_AUTO's sample counters on the device
    float* pool = nullptr;          // [npages][5][32]
    int32_t* pt[2] = { nullptr, nullptr };   // [n][nb] page tables, current and next
    int pt_cur = 0;
    int32_t* freelist = nullptr;    // [npages] ascending free pages as of the last update
    uint32_t* stamp = nullptr;      // [npages] frame stamp of the last table that named the page
    uint32_t stamp_now = 0;
    int32_t* page_scratch = nullptr;   // the free list's bookkeeping (pool_state_words()) | count | tpage[nb] | tindex[nb] | tmask[nb] | tbase[nb + 1] |
                                       // the frame's observation list id[Lp] | zx[Lp] | zy[Lp] | round[Lp] | {count, highest round}
    // ---- split layout (SLAM_MAP_SPLIT, and what SLAM_MAP_AUTO keeps a single-GPU session on while its frames observe most
    // landmarks): means per particle, covariances per covariance class (split_kernels.hip); carved out of the same store
    bool split = false;
    bool dense_split = false;       // AUTO's layout for dense frames is split (else rows)
    float* mean[2] = { nullptr, nullptr };   // [cap][2][Lp]: mean[0] and cov share one half of the store, mean[1] starts the other
    float* cov = nullptr;           // [cap][3][Lp], updated in place once per class and frame
    float* covx = nullptr;          // [cap][2][Lp]: the determinant terms of the same covariances (behind mean[1])
    int sp_base = 0;                // the half of the store that holds mean[0] and cov
    int sp_cur = 0;                 // mean / class buffer of the current particles
    int32_t* cls[2] = { nullptr, nullptr };    // [cap]
    int32_t* live[2] = { nullptr, nullptr };   // [cap] the classes in use, current list and next
    int32_t* cov_cnt = nullptr;     // [3] list lengths, rotating (see cov_update_body.h)
    uint32_t* cstamp = nullptr;     // [cap]
    uint32_t cstamp_now = 0, cls_epoch = 0;
    int live_cur = 0, cov_phase = 0;
    // sharded: a row that arrives from another rank gets a class of its own; the numbers come from a free list on the device
    // (split_kernels.hip: class_free_list_kernel), handed out by the host: a fresh list holds at least recv_cap numbers
    int32_t* cls_free = nullptr;    // [cap]
    int32_t* cls_fs = nullptr;      // two words of the list kernel's bookkeeping
    int64_t cls_cursor = 0;         // entries of the current list handed out so far (beyond its guaranteed length: make a new one)
    uint32_t cls_appended = 0;      // classes appended to the list so far in this epoch (what cov_update_body's `mark` carries)
    void* split_scratch = nullptr;  // flags, prefix sums of a rows -> split move
    // ---- survivor rows (one GPU, split, resampling every frame): the fused front launch of a frame writes
    // no mean row, a launch behind the resample writes the rows of the particles it kept (materialise).  Until the next step the
    // session keeps what the frame's update started from — the previous mean rows, gather index, classes and the frame's poses
    // are intact anyway; the observation table and the prior rows of the classes it updates are copied — so that settle_means
    // can still write every row when something other than the next eligible frame wants to look.
    bool surv_can = false;          // the session can have such frames; the buffers are made when the first one comes up
    bool surv_failed = false;       // ... and could not be had: it writes every row, as ever
    float* surv_store = nullptr;    // the one allocation behind the next four
    float* save_cov = nullptr;      // [cap][3][Lp] prior rows of the classes the last frame updated (cov_update_body)
    float* save_covx = nullptr;     // [cap][2][Lp]
    float* obs_save = nullptr;      // [2][Lp] the last frame's observation table
    uint32_t* survivor = nullptr;   // [n] == surv_stamp: the last resample kept the particle
    uint32_t surv_stamp = 0;
    struct {                        // the frame whose rows are not all written yet (pending)
        bool pending = false;
        const float* mean_in = nullptr;
        float* mean_out = nullptr;
        const int32_t *anc = nullptr, *cls_in = nullptr;
        const float* pose = nullptr;
        int group = 0;
    } surv;
    bool gated = false;             // cfg.resample_ess_frac in (0, 1): a frame resamples only when its ESS is low
    int64_t frames_resampled = 0;   // (as far as the host has looked: one frame behind)
    // slam_pf_refine_set: sweeps > 0: the front launch of a frame is motion + refine (refine_kernels.hip), never the fused front
    float refine_step_xy = 0.0f, refine_step_theta = 0.0f;
    int refine_sweeps = 0;
    // slam_pf_meas_cov_set (rows only): a full 2x2 measurement covariance — the landmark update of every frame runs under it
    // (update_noise), a launch of its own (never the fused front)
    bool aniso = false;
    float meas_cov[3] = { 0.0f, 0.0f, 0.0f };
    // slam_pf_assoc_set (rows only, one GPU): the frame's observations are detections without identity — every frame that uses
    // observations runs the association and then the update under its table, two launches of their own (never the fused front)
    bool assoc_on = false;
    float assoc_gate = 0.0f, assoc_new_gate = 0.0f;
    int assoc_create = 0;
    // slam_pf_assoc_cov_set: association under a full 2x2 Q — the same two launches under it (update_noise; assoc_cov is read only
    // while assoc_aniso is set; `aniso` above stays false)
    bool assoc_aniso = false;
    float assoc_cov[3] = { 0.0f, 0.0f, 0.0f };
    uint8_t* assoc_tab = nullptr;     // [n][Lp] the last frame's table, indexed like `score`; made by the first slam_pf_assoc_set
    int32_t* assoc_stats = nullptr;   // [n][3], behind the table in the same allocation
    // slam_pf_prune_set (only while association is on): one evidence byte per (particle, landmark slot) beside the rows, brought up
    // to date behind every associating update (slam_landmark_evidence_dev); ev[map_cur] belongs to map[map_cur] — the two flip together
    bool prune_on = false;
    int prune_hit = 0, prune_miss = 0, prune_cmax = 0;
    float prune_range = 0.0f;
    uint8_t* ev[2] = { nullptr, nullptr };   // [n][Lp] each, one allocation made by the first slam_pf_prune_set that switches on
    int32_t* ev_stats = nullptr;             // [n][2] pruned, seen after pruning (the last frame that ran the stage), behind them
    // slam_pf_detect_set (only while association is on): every observing frame makes its detections from the engine's scan
    // (slam_detect_scan_dev), issued in front of the frame's first launch
    bool detect_on = false;
    slam_detect_params detect_params{};
    // SLAM_MAP_AUTO: the session watches how many landmarks the frames observe (RES_OBS) and moves between split and
    // split pages while it runs (between rows and pages when it could not have the split layout's tables)
    int layout_cfg = SLAM_MAP_AUTO;
    uint32_t obs_seq_issued = 0, obs_seq_seen = 0;
    int votes_pages = 0, votes_rows = 0;
    bool auto_stuck = false;        // a conversion ran out of memory: stay where we are
    int64_t conversions = 0;
    bool counted = false;           // this session holds the engine's one session slot
    bool last_ekf = false;          // the last frame ran the landmark update (its log-likelihoods are in the engine)
    int32_t* sel = nullptr;         // grow-only scratch of slam_pf_get_map_rows_host: chosen particles | their source rows
    int sel_cap = 0;
    float* conv_tmp = nullptr;      // grow-only scratch of a move off pages (convert_to_rows, convert_split_pages_to_split)
    size_t conv_floats = 0;
};

namespace {

hipError_t dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 4); }

// a word of the mapped result block as the host / the device sees it
int32_t* host_word(const slam_pf* pf, ResWord w) { return reinterpret_cast<int32_t*>(pf->h_res) + w; }
int32_t* dev_word(const slam_pf* pf, ResWord w) { return reinterpret_cast<int32_t*>(pf->d_hres) + w; }

int wait_stream(slam_pf* pf)
{
    if (pf->comm) return comm_wait_stream(pf->comm);
    SLAM_HIP_TRY(pf->e, hipStreamSynchronize(pf->e->stream));
    return SLAM_OK;
}

// Grow-only device scratch: *buf is replaced by one of `bytes` bytes.  Work in flight may still read the old one, so the stream
// is drained first (`drain_always`: also when there is none).  Memory not to be had: SLAM_OK with *buf == nullptr, the caller decides.
int replace_scratch(slam_pf* pf, void** buf, size_t bytes, bool drain_always)
{
    if (*buf || drain_always)
        if (int rc = wait_stream(pf)) return rc;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr;
    if (hipMalloc(buf, bytes) != hipSuccess) {
        (void)hipGetLastError();
        *buf = nullptr;
    }
    return SLAM_OK;
}

int grow(slam_pf* pf, float** buf, size_t* have, size_t want)
{
    if (want <= *have) return SLAM_OK;
    const size_t cap = want > 2 * *have ? want + want / 2 : 2 * *have;
    if (int rc = replace_scratch(pf, (void**)buf, cap * sizeof(float), true)) return rc;
    *have = *buf ? cap : 0;
    return *buf ? SLAM_OK : slam_engine_fail_hip(pf->e, hipErrorOutOfMemory, "exchange buffer");
}

// the scratch rows of a move off pages; not to be had: the session stays where it is (auto_stuck, no error)
int conversion_scratch(slam_pf* pf, size_t floats)
{
    if (pf->conv_floats >= floats) return SLAM_OK;   // (an alloc + free per move would serialise the frame every time)
    if (int rc = replace_scratch(pf, (void**)&pf->conv_tmp, floats * 4, false)) return rc;
    pf->conv_floats = pf->conv_tmp ? floats : 0;
    if (!pf->conv_tmp) pf->auto_stuck = true;
    return SLAM_OK;
}

// a new free list when the old one runs short (decided on the device; the pages in use carry the last stamp)
int issue_free_list(slam_pf* pf)
{
    SLAM_HIP_TRY(pf->e, launch_free_list(pf->e->stream, pf->stamp, pf->npages, pf->stamp_now, pf->freelist, pf->page_scratch,
                                         dev_word(pf, RES_SHORT_LIST)));
    return SLAM_OK;
}

float* split_pool(const slam_pf* pf);
PageGeom split_geom(const slam_pf* pf);
PagePool page_pool(const slam_pf* pf);
ClassStore class_store(const slam_pf* pf);

// Survivor rows: the mean rows of the pending frame, from the inputs it started from (the same device functions as its front
// launch: the same bits) — for the particles the resample kept (filtered), or all of them.
int materialise(slam_pf* pf, bool filtered)
{
    const size_t sn = (size_t)pf->n;
    SplitIO sio{};
    sio.cov = pf->save_cov;
    sio.cov_stride = 3 * (int64_t)pf->Lp;
    sio.covx = pf->save_covx;
    sio.covx_stride = 2 * (int64_t)pf->Lp;
    sio.cls_in = pf->surv.cls_in;
    return slam_ekf_materialise_dev(pf->e, pf->surv.mean_in, pf->surv.mean_out, 2 * (int64_t)pf->Lp, pf->Lp, pf->L, pf->obs_save,
                                    pf->surv.pose, pf->surv.pose + sn, pf->surv.pose + 2 * sn, pf->surv.anc, pf->n, pf->cfg.meas_var, &sio,
                                    filtered ? pf->survivor : nullptr, pf->surv_stamp, pf->surv.group);
}

// The buffers of the mode, made in front of the first frame that wants them (a session whose switch stays off, or that never
// has such a frame, does not pay for them): one allocation, zeroed on the stream.
bool survivor_buffers(slam_pf* pf)
{
    if (pf->surv_store) return true;
    if (!pf->surv_can || pf->surv_failed) return false;
    const size_t unit = (size_t)pf->Lp * (size_t)pf->cap, words = 5 * unit + 2 * (size_t)pf->Lp + (size_t)pf->n;
    if (hipMalloc((void**)&pf->surv_store, words * 4) != hipSuccess ||
        hipMemsetAsync(pf->surv_store, 0, words * 4, pf->e->stream) != hipSuccess) {
        (void)hipGetLastError();
        if (pf->surv_store) (void)hipFree(pf->surv_store);
        pf->surv_store = nullptr;
        pf->surv_failed = true;
        return false;
    }
    pf->save_cov = pf->surv_store;
    pf->save_covx = pf->save_cov + 3 * unit;
    pf->obs_save = pf->save_covx + 2 * unit;
    pf->survivor = reinterpret_cast<uint32_t*>(pf->obs_save + 2 * (size_t)pf->Lp);
    return true;
}

// Before anything but the next eligible frame sees a mean row: after this the buffers hold what a frame that wrote every row
// leaves.  Called by every entry that reads or moves mean rows or hands out their address (slam_pf_get_map_rows_host reads
// through the pending gather — survivors only — and does not need it).
int settle_means(slam_pf* pf)
{
    if (!pf->surv.pending) return SLAM_OK;
    pf->surv.pending = false;
    return materialise(pf, false);
}

// Pruning: the evidence of the current maps, from scratch — a map that is there is trusted (seen: cmax, else 0).  At the switch,
// and whenever the session's maps are replaced wholesale while pruning is on.
int evidence_from_maps(slam_pf* pf)
{
    if (!pf->prune_on) return SLAM_OK;
    return slam_evidence_init_dev(pf->e, pf->map[pf->map_cur], 5 * (int64_t)pf->Lp, pf->Lp, pf->L, pf->n, pf->ev[pf->map_cur], pf->Lp,
                                  pf->prune_cmax);
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
        if (int rc = slam_migrate_pack_paged(e, n, pf->rank, G, plan, pf->pose[pf->cur], n, mp, (split ? 2 : 5) * (int64_t)pf->Lp, pf->Lp, L,
                                             pf->sbuf, pf->paged ? pf->pt[pf->pt_cur] : nullptr, pf->nb, split ? pf->cov : nullptr,
                                             split ? pf->cls[pf->sp_cur] : nullptr, spages ? &geom : nullptr))
            return rc;
    if (int rc = comm_all_to_all_f32(pf->comm, pf->sbuf, sfl, pf->rbuf, rfl)) return rc;
    if (rtot && split) {
        // every received row becomes a class of its own (it brings its covariances along); its number comes from the free list
        // of classes on the device, made anew from the stamps when its guaranteed length — a rank's staging rows: at most n
        // classes are in use — is used up (SLAM_SPLIT_CLASS_ROOM: tests make the lists short)
        const char* room_env = getenv("SLAM_SPLIT_CLASS_ROOM");
        const int64_t room = room_env && atoi(room_env) > 0 && atoi(room_env) < pf->recv_cap ? atoi(room_env) : pf->recv_cap;
        const ProfScope prof(e, SLAM_PROF_UNPACK);
        if (pf->cls_cursor + rtot > room) {
            SLAM_HIP_TRY(e, launch_class_free_list(e->stream, pf->cstamp, pf->cap, pf->cstamp_now, pf->cls_free, pf->cls_fs));
            pf->cls_cursor = 0;
        }
        if (spages) {   // the means onto fresh pages (a new free list first if the old one runs short), table rows n .. n + rtot - 1
            SLAM_HIP_TRY(e, launch_pool_reserve(e->stream, pf->page_scratch, rtot * pf->nb));
            if (int rc = issue_free_list(pf)) return rc;
            SLAM_HIP_TRY(e, launch_migrate_unpack_split_pages(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, page_pool(pf),
                                                              class_store(pf), L, pf->cfg.meas_var, pf->cls_free, (int)pf->cls_cursor));
        } else
            SLAM_HIP_TRY(e, launch_migrate_unpack_split(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, pf->mean[pf->sp_cur],
                                                        class_store(pf), L, pf->cfg.meas_var, pf->cls_free, (int)pf->cls_cursor));
        pf->cls_cursor += rtot;
        pf->cls_appended += (uint32_t)rtot;
    } else if (rtot && pf->paged) {
        // fresh pages for the received rows (a new free list first if the old one runs short), table rows n .. n + rtot - 1
        const ProfScope prof(e, SLAM_PROF_UNPACK);
        SLAM_HIP_TRY(e, launch_pool_reserve(e->stream, pf->page_scratch, rtot * pf->nb));
        if (int rc = issue_free_list(pf)) return rc;
        SLAM_HIP_TRY(e, launch_migrate_unpack_paged(e->stream, pf->rbuf, (int)rtot, n, pf->pose_stage, pf->cap, page_pool(pf), L));
    } else if (rtot) {
        if (int rc = slam_migrate_unpack_dev(e, pf->rbuf, G, rcnt, n, pf->pose_stage, pf->cap,
                                             L ? pf->map[pf->map_cur] : nullptr, 5 * (int64_t)pf->Lp, pf->Lp, L))
            return rc;
    }
    return SLAM_OK;
}

// Every slam_pf_* call on a sharded session is collective: a rank that fails one alone (an error of its own, not a verdict
// every rank reaches together) must not leave the others waiting inside it — it gives up for good (comm_abort), the peers get
// SLAM_ERR_COMM at once instead of after SLAM_COMM_TIMEOUT_S.
int collective_result(slam_pf* pf, int rc)
{
    // (argument checks come before anything collective and are the same on every rank of a sane host: no abort for those)
    if (rc != SLAM_OK && rc != SLAM_ERR_INVALID_ARG && rc != SLAM_ERR_NOT_READY && pf && pf->comm) (void)comm_abort(pf->comm);
    return rc;
}

int finish_exchange(slam_pf* pf)
{
    if (!pf->exchange_pending) return SLAM_OK;
    pf->exchange_pending = false;
    return migrate(pf);
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

// wait for a result kernel's sequence number in mapped host memory
int wait_result(slam_pf* pf, uint32_t seq)
{
    const volatile uint32_t* h_seq = reinterpret_cast<const volatile uint32_t*>(host_word(pf, RES_SEQ));
    return slam_engine_wait_flag(pf->e, pf->comm, h_seq, seq, "result flag");
}

int gathered_copy_out(slam_pf* pf, const float* d_src, const int32_t* idx, float* h_dst, float* d_tmp)
{
    // d_src gathered through idx on the device (idx == nullptr: as is), then copied back
    if (idx) {
        int rc = slam_gather_f32_dev(pf->e, d_src, idx, pf->n, d_tmp);
        if (rc != SLAM_OK) return rc;
        d_src = d_tmp;
    }
    if (int rc = slam_engine_sync(pf->e)) return rc;
    return hipMemcpy(h_dst, d_src, sizeof(float) * (size_t)pf->n, hipMemcpyDeviceToHost) == hipSuccess ? SLAM_OK
                                                                                                      : SLAM_ERR_HIP;
}

// ---- the landmark maps live in ONE allocation `store` of 2 x cap x 5 x Lp floats, seen either as two row buffers
// (map[0] = the first half, map[1] = the second) or as a pool of 2 x cap x nb pages (the same bytes: a page is 5 x 32 floats,
// a row nb of them).  The page tables, free list and stamps exist only for sessions that may be on pages.
bool alloc_store(slam_pf* pf)
{
    const size_t half = 5 * (size_t)pf->Lp * (size_t)pf->cap;   // floats
    if (dev_alloc((void**)&pf->store, 2 * half * 4) != hipSuccess) {
        (void)hipGetLastError();
        pf->store = nullptr;
        return false;
    }
    pf->map[0] = pf->store;
    pf->map[1] = pf->store + half;
    pf->pool = pf->store;
    return true;
}

void free_page_tables(slam_pf* pf)
{
    for (void** p : { (void**)&pf->pt[0], (void**)&pf->pt[1], (void**)&pf->freelist, (void**)&pf->stamp, (void**)&pf->page_scratch,
                      (void**)&pf->votes }) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

bool alloc_page_tables(slam_pf* pf)
{
    const size_t P = (size_t)pf->npages, words = 4 * (size_t)pf->nb + 2 + (size_t)pool_state_words() + 4 * (size_t)pf->Lp + 2;
    const bool ok = dev_alloc((void**)&pf->freelist, P * 4) == hipSuccess && dev_alloc((void**)&pf->stamp, P * 4) == hipSuccess &&
                    hipMemset(pf->stamp, 0, P * 4) == hipSuccess && dev_alloc((void**)&pf->page_scratch, words * 4) == hipSuccess &&
                    hipMemset(pf->page_scratch, 0, words * 4) == hipSuccess &&
                    dev_alloc((void**)&pf->pt[0], (size_t)pf->cap * pf->nb * 4) == hipSuccess &&
                    dev_alloc((void**)&pf->pt[1], (size_t)pf->cap * pf->nb * 4) == hipSuccess &&
                    dev_alloc((void**)&pf->votes, 2 * 4) == hipSuccess && hipMemset(pf->votes, 0, 2 * 4) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        free_page_tables(pf);
    }
    return ok;
}

// rows -> pages while the session runs: ONE kernel, stream-ordered, no allocation.  The current rows sit in one half of the
// store (before the pending gather); they are written as pages into the OTHER half — page (other half's first page) + r * nb
// + b behind identity tables, so the pending gather index means the same thing afterwards — and the half they came from
// becomes free pages.
// Sharded: when the exchange of the last frame has already been completed (a map getter between two frames does that), the
// pending gather index also names rows of the staging tail, n .. n + rows_received - 1: they move with the rest.
int rows_to_convert(const slam_pf* pf)
{
    return pf->n + (pf->comm && pf->has_anc && !pf->exchange_pending ? pf->rows_received : 0);
}

int convert_to_pages(slam_pf* pf)
{
    slam_engine* e = pf->e;
    const int mc = pf->map_cur;
    const int page_base = (1 - mc) * pf->cap * pf->nb;
    pf->pt_cur = 0;
    SLAM_HIP_TRY(e, launch_pages_from_rows(e->stream, pf->map[mc], 5 * (int64_t)pf->Lp, pf->Lp, pf->L, rows_to_convert(pf), page_pool(pf),
                                           page_base));
    pf->paged = true;
    pf->conversions++;
    return SLAM_OK;
}

// pages -> rows: the pages lie anywhere in the store, a row buffer is one contiguous half of it, so the rows are put
// together in a scratch buffer first (row r = the pages table row r names, again before the pending gather) and copied
// into the first half.  While it runs this takes half as much memory again; when that is not to be had the session stays
// on pages.
int convert_to_rows(slam_pf* pf)
{
    slam_engine* e = pf->e;
    const int nrows = rows_to_convert(pf);
    const size_t used = 5 * (size_t)pf->Lp * (size_t)nrows;
    if (int rc = conversion_scratch(pf, used)) return rc;
    if (!pf->conv_tmp) return SLAM_OK;
    // stream-ordered: pages -> scratch rows -> the first half of the store (the scratch is read before anything else writes it)
    SLAM_HIP_TRY(e, launch_rows_from_pages(e->stream, page_pool(pf), nullptr, nrows, pf->conv_tmp, 5 * (int64_t)pf->Lp, pf->Lp, pf->L));
    SLAM_HIP_TRY(e, hipMemcpyAsync(pf->map[0], pf->conv_tmp, used * 4, hipMemcpyDeviceToDevice, e->stream));
    pf->map_cur = 0;
    pf->paged = false;
    pf->conversions++;
    return SLAM_OK;
}

// ---- split layout: tables, placement in the store, moves
void free_split_tables(slam_pf* pf)
{
    for (void** p : { (void**)&pf->cls[0], (void**)&pf->cls[1], (void**)&pf->live[0], (void**)&pf->live[1], (void**)&pf->cov_cnt,
                      (void**)&pf->cstamp, &pf->split_scratch, (void**)&pf->cls_free, (void**)&pf->cls_fs }) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
}

bool alloc_split_tables(slam_pf* pf)
{
    const size_t cap = (size_t)pf->cap;
    bool ok = true;
    for (int b = 0; b < 2; ++b)
        ok = ok && dev_alloc((void**)&pf->cls[b], cap * 4) == hipSuccess && dev_alloc((void**)&pf->live[b], cap * 4) == hipSuccess;
    ok = ok && dev_alloc((void**)&pf->cov_cnt, 16) == hipSuccess && hipMemset(pf->cov_cnt, 0, 16) == hipSuccess &&
         dev_alloc((void**)&pf->cstamp, cap * 4) == hipSuccess && hipMemset(pf->cstamp, 0, cap * 4) == hipSuccess &&
         dev_alloc(&pf->split_scratch, split_scratch_words(pf->cap) * 4) == hipSuccess &&
         dev_alloc((void**)&pf->cls_fs, 8) == hipSuccess && hipMemset(pf->cls_fs, 0, 8) == hipSuccess &&
         (!pf->comm || dev_alloc((void**)&pf->cls_free, cap * 4) == hipSuccess);
    if (!ok) {
        (void)hipGetLastError();
        free_split_tables(pf);
    }
    return ok;
}

// mean[0] and cov take the half `base` of the store (2 + 3 of its 5 units), mean[1] and covx (2 + 2) the other half
void place_split(slam_pf* pf, int base)
{
    const size_t half = 5 * (size_t)pf->Lp * (size_t)pf->cap, unit = (size_t)pf->Lp * (size_t)pf->cap;
    pf->sp_base = base;
    pf->mean[0] = pf->store + (size_t)base * half;
    pf->cov = pf->mean[0] + 2 * unit;
    pf->mean[1] = pf->store + (size_t)(1 - base) * half;
    pf->covx = pf->mean[1] + 2 * unit;
}

// ---- SPLIT PAGES (paged && split): the means on copy-on-write pages of two planes (256 bytes), the covariances per class as
// on the split layout.  The pages live in the session's two mean buffers (2 x cap x nb pages, exactly their size), which are
// not neighbours in the store: pages below cap x nb in the buffer at the lower address, the others in the other one.
float* split_pool(const slam_pf* pf) { return pf->mean[0] < pf->mean[1] ? pf->mean[0] : pf->mean[1]; }
PageGeom split_geom(const slam_pf* pf)
{
    PageGeom g;
    g.planes = 2;
    g.half_pages = (int64_t)pf->cap * pf->nb;
    const float *lo = split_pool(pf), *hi = pf->mean[0] < pf->mean[1] ? pf->mean[1] : pf->mean[0];
    g.gap = (hi - lo) - g.half_pages * 2 * kPageLandmarks;
    return g;
}

// the page pool and the class store as the launchers off the frame path take them (kernels.h): the current table, the current
// class buffer and list, the stamps of the last update
PagePool page_pool(const slam_pf* pf)
{
    return PagePool{ pf->split ? split_pool(pf) : pf->pool, pf->split ? split_geom(pf) : PageGeom(), pf->pt[pf->pt_cur], pf->nb,
                     pf->freelist, pf->npages, pf->page_scratch, pf->stamp, pf->stamp_now };
}
ClassStore class_store(const slam_pf* pf)
{
    return ClassStore{ pf->cov, pf->covx, pf->cls[pf->sp_cur], pf->Lp, pf->cstamp, pf->cstamp_now, pf->live[pf->live_cur],
                       pf->cov_cnt + pf->cov_phase };
}

// a new set of classes is about to be made (set_map, reset, rows -> split): lists and counters start afresh
void split_new_epoch(slam_pf* pf)
{
    pf->cls_epoch++;
    pf->cstamp_now++;
    pf->live_cur = 0;
    pf->cov_phase = 0;
    pf->cls_appended = 0;
    pf->cls_cursor = (int64_t)1 << 40;   // no list of free class numbers yet: the first arrivals make one
}

// nrows rows (as given, any strides) -> means + classes + class rows in the buffers of the current placement
int split_from_rows(slam_pf* pf, const float* d_rows, int64_t row_stride, int plane_stride, int nrows)
{
    slam_engine* e = pf->e;
    split_new_epoch(pf);
    SLAM_HIP_TRY(e, launch_split_from_rows(e->stream, d_rows, row_stride, plane_stride, pf->L, nrows, pf->mean[pf->sp_cur], class_store(pf),
                                           pf->cfg.meas_var, dev_word(pf, RES_LIVE), pf->cls_epoch, pf->split_scratch));
    return SLAM_OK;
}

// rows -> split while the session runs: stream-ordered, no allocation.  The rows sit in one half of the store; the means and
// the class rows go into the OTHER half, and the half the rows came from becomes the second mean buffer.
int convert_rows_to_split(slam_pf* pf)
{
    const int mc = pf->map_cur;
    place_split(pf, 1 - mc);
    pf->sp_cur = 0;
    if (int rc = split_from_rows(pf, pf->map[mc], 5 * (int64_t)pf->Lp, pf->Lp, rows_to_convert(pf))) return rc;
    pf->split = true;
    pf->conversions++;
    return SLAM_OK;
}

// split -> split pages: the means of the current buffer become pages in the OTHER mean buffer (identity tables, shifted),
// the buffer they came from becomes free pages; classes and covariances stay where they are.  One stream-ordered launch.
int split_means_to_pages(slam_pf* pf)
{
    slam_engine* e = pf->e;
    const float* src = pf->mean[pf->sp_cur];
    const float* dst = pf->mean[1 - pf->sp_cur];
    const int page_base = dst == split_pool(pf) ? 0 : pf->cap * pf->nb;
    pf->pt_cur = 0;
    // (sharded: rows_to_convert takes the staging tail along when the exchange of the last frame has been completed already)
    SLAM_HIP_TRY(e, launch_pages_from_rows(e->stream, src, 2 * (int64_t)pf->Lp, pf->Lp, pf->L, rows_to_convert(pf), page_pool(pf), page_base));
    pf->paged = true;
    return SLAM_OK;
}

int convert_split_to_split_pages(slam_pf* pf)
{
    if (int rc = split_means_to_pages(pf)) return rc;
    pf->conversions++;
    return SLAM_OK;
}

// split pages -> split: the pages lie anywhere in the two mean buffers, so the rows are put together in the scratch buffer of
// convert_to_rows first and copied into mean[0]
int convert_split_pages_to_split(slam_pf* pf)
{
    slam_engine* e = pf->e;
    const int nrows = rows_to_convert(pf);
    const size_t used = 2 * (size_t)pf->Lp * (size_t)nrows;
    if (int rc = conversion_scratch(pf, used)) return rc;
    if (!pf->conv_tmp) return SLAM_OK;
    SLAM_HIP_TRY(e, launch_rows_from_pages(e->stream, page_pool(pf), nullptr, nrows, pf->conv_tmp, 2 * (int64_t)pf->Lp, pf->Lp, pf->L));
    SLAM_HIP_TRY(e, hipMemcpyAsync(pf->mean[0], pf->conv_tmp, used * 4, hipMemcpyDeviceToDevice, e->stream));
    if (pf->sp_cur == 1) SLAM_HIP_TRY(e, hipMemcpyAsync(pf->cls[0], pf->cls[1], (size_t)nrows * 4, hipMemcpyDeviceToDevice, e->stream));
    pf->sp_cur = 0;
    pf->paged = false;
    pf->conversions++;
    return SLAM_OK;
}

// SLAM_MAP_AUTO, at the start of a frame: look at the counts that have arrived since the last look (no waiting) and move
// when the last three agree.  Pages pay when a frame observes at most two sevenths of the landmarks (a resampling frame on
// rows rewrites every row in full); rows / split maps pay when it observes more than three eighths (most pages are touched
// anyway and the row kernels are faster at that; the measured change-over is at 0.28-0.33).  Results do not depend on the layout, so the ranks of a sharded session may decide apart.
int auto_layout(slam_pf* pf)
{
    if (pf->layout_cfg != SLAM_MAP_AUTO || pf->L == 0 || pf->auto_stuck) return SLAM_OK;
    const volatile uint32_t* h_seq = reinterpret_cast<const volatile uint32_t*>(host_word(pf, RES_OBS_SEQ));
    // The first frames of a session WAIT for the sample of the frame before (it is taken early in that frame: the wait is
    // about one motion + score launch), so that a session settles on its layout within its first four frames however far
    // the host runs ahead of the device; later looks never wait.
    if (pf->frame <= 3 && pf->obs_seq_issued != pf->obs_seq_seen) {
        if (pf->comm) {
            if (int rc = comm_wait_flag(pf->comm, h_seq, pf->obs_seq_issued)) return rc;
        } else
            (void)slam_spin_flag(h_seq, pf->obs_seq_issued);   // (never showed up: this look finds nothing new, that is all)
    }
    const uint32_t seq = __atomic_load_n(h_seq, __ATOMIC_ACQUIRE);
    if (seq == pf->obs_seq_seen) return SLAM_OK;
    pf->obs_seq_seen = seq;
    pf->votes_pages = *host_word(pf, RES_VOTES_PAGES);   // samples in a row (counted on the device, so none is missed however far the host runs ahead)
    pf->votes_rows = *host_word(pf, RES_VOTES_ROWS);
    if ((!pf->paged && pf->votes_pages >= 3) || (pf->paged && pf->votes_rows >= 3))
        if (int rc = settle_means(pf)) return rc;   // a move reads every row
    if (!pf->paged && pf->votes_pages >= 3) {
        if (pf->split) return convert_split_to_split_pages(pf);   // the means go onto pages, the classes stay
        return convert_to_pages(pf);
    }
    if (pf->paged && pf->votes_rows >= 3) {
        if (pf->split) return convert_split_pages_to_split(pf);
        if (int rc = convert_to_rows(pf)) return rc;
        if (!pf->paged && pf->dense_split) return convert_rows_to_split(pf);
    }
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
        pf->dense_split = have && pf->layout_cfg == SLAM_MAP_AUTO;
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
         dev_alloc((void**)&pf->res_dev, 128) == hipSuccess && dev_alloc((void**)&pf->sums_acc, 128) == hipSuccess &&
         dev_alloc(&pf->res_all, 128 * G) == hipSuccess &&
         hipMemset(pf->sums_acc, 0, 128) == hipSuccess;
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

// ---- one frame (pf_step_impl): the arguments its launches take, then its stages in the order they are issued
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
    ca.cov_stride = 3 * (int64_t)pf->Lp;
    ca.covx = pf->covx;
    ca.covx_stride = 2 * (int64_t)pf->Lp;
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
    sio.cov_stride = 3 * (int64_t)pf->Lp;
    sio.covx = pf->covx;
    sio.covx_stride = 2 * (int64_t)pf->Lp;
    sio.cls_in = pf->cls[pf->sp_cur];
    sio.cls_out = pf->cls[1 - pf->sp_cur];
    sio.cstamp = pf->cstamp;
    sio.stamp_now = pf->cstamp_now + 1;
    return sio;
}

// What a frame is, decided once behind auto_layout (nothing later changes the layout), and what its stages leave for the next
struct FrameFacts {
    bool ekf;          // the host asks for the landmark update ...
    bool observing;    // ... and the engine holds an observation table for these landmarks
    bool sample_obs;   // SLAM_MAP_AUTO takes its sample of the number of observed landmarks in this frame
    const int32_t* anc;   // the pending gather of the last resample (nullptr: none)
    const float* src;     // poses: current -> next
    float* dst;
    int64_t first_id;
    // page_scratch: the free list's bookkeeping | count | tpage[nb] | tindex[nb] | tmask[nb] | tbase[nb + 1] | the observation list
    int32_t *count, *tpage, *tindex, *tmask, *tbase;
    ObsListOut lo;     // the list form of the paged update (one lane per observation) whenever a list can be made
    // ---- left by the stages
    bool paged_listed;   // front: the page list is out, the free list rides with the scorer
    bool fused;          // front: the landmark update went out with the score
    bool survivors;      // front: ... and wrote no mean row (survivor rows): the resample marks whom it keeps, a launch behind it writes their rows
    bool weighted;       // front: ... and made the log-weights and their block maxima as well: no weights' launch
    bool classes_due;    // update: the classes' update (cov, cov_bound) has its arguments and still wants a launch to ride in: the scan's
    CovArgs cov;
    int cov_bound;
    bool in_place;       // gate: the last frame kept its population, the maps have not moved
};

FrameFacts frame_facts(const slam_pf* pf, int use_observations)
{
    FrameFacts f{};
    f.ekf = pf->L > 0 && use_observations;
    f.observing = f.ekf && pf->e->obs_nlandmarks == pf->L;
    // SLAM_MAP_AUTO samples the number of observed landmarks: every frame at the start and while the counts speak against
    // the current layout, every 8th frame otherwise
    f.sample_obs = pf->layout_cfg == SLAM_MAP_AUTO && !pf->auto_stuck && f.observing &&
                   (pf->frame < 8 || (pf->frame & 7u) == 0 || (pf->paged ? pf->votes_rows : pf->votes_pages) > 0);
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

// 1 + 2. motion (+ the fused gather of the previous resample) and scan-match score, one launch.  Sharded: the ancestors' poses come
// out of the array of every rank's poses: it needs nothing from the exchange and keeps the GPU busy while the host picks up the plan.
int front_stage(slam_pf* pf, FrameFacts& f, int slot, const float dp[3])
{
    slam_engine* e = pf->e;
    slam_comm* comm = pf->comm;
    const int n = pf->n, cur = pf->cur;
    const size_t sn = (size_t)n;
    float* dst = f.dst;
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
        const float* ps = f.src;
        const int32_t* pose_anc = f.anc;
        if (comm && pf->has_anc) {
            if (int rc = comm_all_gather_finish(comm)) return rc;
            ps = pf->pose_all;
            pose_anc = pf->pose_idx[cur];
        }
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
        const float* ps = f.src;
        const int32_t* pose_anc = f.anc;
        if (comm) {
            if (int rc = comm_all_gather_finish(comm)) return rc;
            ps = pf->pose_all;
            pose_anc = pf->pose_idx[cur];
        }
        const SplitIO sio = pf->split ? split_io(pf, comm ? 1 : 0, comm ? f.anc : nullptr) : SplitIO{};
        const float* map_in = pf->split ? pf->mean[pf->sp_cur] : pf->map[pf->map_cur];
        float* map_out = pf->split ? pf->mean[1 - pf->sp_cur] : pf->map[1 - pf->map_cur];
        // (a survivor-rows frame may come back with its weights made as well: one workgroup scores and updates a particle)
        const slam_front_weights fw{ pf->cfg.score_gain, pf->logw, &f.weighted };
        if (int rc = slam_frame_front_dev(e, slot, ps, ps + sn, ps + 2 * sn, pose_anc, dst, dst + sn, dst + 2 * sn, n, f.first_id, dp,
                                          pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->score, pf->count, map_in, map_out,
                                          (pf->split ? 2 : 5) * (int64_t)pf->Lp, pf->Lp, pf->L, pf->cfg.meas_var, &f.fused,
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
    if (comm && pf->has_anc) {
        if (int rc = comm_all_gather_finish(comm)) return rc;
        const float* pa = pf->pose_all;
        return slam_motion_score_dev(e, slot, pa, pa + sn, pa + 2 * sn, pf->pose_idx[cur], dst, dst + sn, dst + 2 * sn, n, f.first_id,
                                     dp, pf->cfg.sigma, pf->cfg.seed, pf->frame, pf->score, pf->count);
    }
    bool rode = false;
    if (int rc = slam_motion_score_rider_dev(e, slot, f.src, f.src + sn, f.src + 2 * sn, f.anc, dst, dst + sn, dst + 2 * sn, n, f.first_id,
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
    if (pf->assoc_on ? pf->assoc_aniso : pf->aniso) return slam_meas_noise{ 0.0f, pf->assoc_on ? pf->assoc_cov : pf->meas_cov, true };
    return slam_meas_noise{ pf->cfg.meas_var, nullptr, false };
}

// 3. per-landmark EKF (+ fused gather) and the weights, one function per storage form.  Rows: in place, out of place, gather only
int update_rows(slam_pf* pf, const FrameFacts& f)
{
    slam_engine* e = pf->e;
    const int n = pf->n, L = pf->L, mc = pf->map_cur, mn = 1 - mc;
    const size_t sn = (size_t)n;
    const int64_t stride = 5 * (int64_t)pf->Lp;
    float* dst = f.dst;
    if (f.ekf) {
        if (f.sample_obs) SLAM_HIP_TRY(e, launch_obs_count(e->stream, e->d_obs_zx, e->d_obs_zy, L, dev_word(pf, RES_OBS), ++pf->obs_seq_issued, pf->votes));
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
            if (pf->prune_on)
                if (int rc = slam_landmark_evidence_dev(e, out, stride, pf->Lp, L, dst, dst + sn, anc, n, pf->assoc_tab, pf->Lp, pf->ev[mc],
                                                        pf->ev[f.in_place ? mc : mn], pf->Lp, pf->prune_hit, pf->prune_miss,
                                                        pf->prune_cmax, pf->prune_range, pf->ev_stats))
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
    return slam_logweight_dev(e, pf->score, nullptr, pf->cfg.score_gain, n, pf->logw, nullptr);
}

int update_split(slam_pf* pf, FrameFacts& f)
{
    slam_engine* e = pf->e;
    const int n = pf->n, L = pf->L, sc = pf->sp_cur;
    const size_t sn = (size_t)n;
    float* dst = f.dst;
    if (f.ekf) {
        if (!f.observing) return SLAM_ERR_NOT_READY;
        if (f.sample_obs) SLAM_HIP_TRY(e, launch_obs_count(e->stream, e->d_obs_zx, e->d_obs_zy, L, dev_word(pf, RES_OBS), ++pf->obs_seq_issued, pf->votes));
        // the particles' update (a frame that kept its population: out of place all the same, through the identity index); behind
        // a sharded fused front: the groups that waited for the exchange — no rows received: the launch would find nothing to do ...
        if (!f.fused || (pf->comm && pf->rows_received > 0)) {
            const SplitIO sio = split_io(pf, f.fused ? 2 : 0, nullptr);
            if (int rc = slam_ekf_split_dev(e, pf->mean[sc], pf->mean[1 - sc], 2 * (int64_t)pf->Lp, pf->Lp, L, dst, dst + sn, dst + 2 * sn,
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
    return slam_logweight_dev(e, pf->score, nullptr, pf->cfg.score_gain, n, pf->logw, nullptr);
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
    if (!f.anc) return slam_logweight_dev(e, pf->score, nullptr, pf->cfg.score_gain, n, pf->logw, nullptr);
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
    return pf->split ? weights_with_classes(pf, 0, false)
                     : slam_logweight_dev(e, pf->score, nullptr, pf->cfg.score_gain, n, pf->logw, nullptr);
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

int pf_step_impl(slam_pf* pf, int slot, const float dp[3], int use_observations, bool* collective_verdict)
{
    slam_engine* e = pf->e;
    if (pf->paged && __atomic_load_n(host_word(pf, RES_SHORT_LIST), __ATOMIC_ACQUIRE) != 0) {
        snprintf(e->err, sizeof e->err, "paged maps: a free list was shorter than the pages reserved from it (pool invariant broken)");
        return SLAM_ERR_CAPACITY;
    }
    if (int rc = auto_layout(pf)) return rc;   // may move the maps to another layout (never changes a result)
    FrameFacts f = frame_facts(pf, use_observations);
    // the detector: in front of the frame's first launch, so that its count has arrived when update_rows' association asks for it
    if (pf->detect_on && pf->assoc_on && f.ekf)
        if (int rc = slam_detect_scan_dev(e, &pf->detect_params, nullptr)) return rc;
    if (int rc = front_stage(pf, f, slot, dp)) return rc;
    if (int rc = gate_and_exchange(pf, f, collective_verdict)) return rc;
    if (int rc = pf->paged ? update_paged(pf, f) : pf->split ? update_split(pf, f) : update_rows(pf, f)) return rc;
    if (int rc = scan_stage(pf, f)) return rc;
    if (int rc = resample_stage(pf, f.dst, f.survivors)) return rc;
    pf->cur = 1 - pf->cur;
    pf->has_anc = true;
    pf->last_ekf = f.ekf;
    pf->frame++;
    return SLAM_OK;
}

int pf_best(slam_pf* pf, float pose[3], float* logw, int32_t* index)
{
    if (!pf || !pose) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    // the log-weights of the last frame belong to pose[cur] BEFORE the pending gather
    const float* p = pf->pose[pf->cur];
    const size_t sn = (size_t)pf->n;
    float r[5];
    if (!pf->comm) {   // one launch, the result lands in mapped host memory: no copy, no stream synchronisation
        const uint32_t seq = ++pf->res_seq;
        SLAM_HIP_TRY(e, launch_best_particle(e->stream, pf->logw, pf->n, p, p + sn, p + 2 * sn, 0, pf->res_dev, pf->d_hres,
                                             reinterpret_cast<uint32_t*>(dev_word(pf, RES_SEQ)), seq));
        if (int rc = wait_result(pf, seq)) return rc;
        memcpy(r, pf->h_res, sizeof r);
    } else {   // every rank's candidate to every rank; the first maximum = the lowest rank = the lowest id
        SLAM_HIP_TRY(e, launch_best_particle(e->stream, pf->logw, pf->n, p, p + sn, p + 2 * sn, (int64_t)pf->rank * pf->n,
                                             pf->res_dev, nullptr, nullptr, 0));
        if (int rc = comm_all_gather(pf->comm, pf->res_dev, pf->res_all, 5 * sizeof(float))) return rc;
        std::vector<float> all(5 * (size_t)pf->world);
        SLAM_HIP_TRY(e, hipMemcpyAsync(all.data(), pf->res_all, all.size() * 4, hipMemcpyDeviceToHost, e->stream));
        if (int rc = comm_wait_stream(pf->comm)) return rc;
        int best = 0;
        for (int q = 1; q < pf->world; ++q)
            if (all[5 * q] > all[5 * best]) best = q;
        memcpy(r, &all[5 * best], sizeof r);
    }
    int32_t gid;
    memcpy(&gid, &r[1], 4);
    for (int k = 0; k < 3; ++k) pose[k] = r[2 + k];
    if (logw) *logw = r[0];
    if (index) *index = gid;
    return SLAM_OK;
}

int pf_mean(slam_pf* pf, float ref_theta, float pose[3])
{
    if (!pf || !pose) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    const size_t sn = (size_t)pf->n;
    const float *x = pf->pose[pf->cur], *y = x + sn, *th = x + 2 * sn;
    const int32_t* idx = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    if (pf->comm && pf->has_anc) {   // the ancestors' poses are in the all-gathered array
        if (int rc = comm_all_gather_finish(pf->comm)) return rc;
        x = pf->pose_all;
        y = x + sn;
        th = x + 2 * sn;
        idx = pf->pose_idx[pf->cur];
    }
    unsigned int* ticket = reinterpret_cast<unsigned int*>(pf->sums_acc + kPoseSumsWeighted);
    // A frame the resample gate kept (its verdict is on its way to mapped host memory: wait for it) left unequal weights:
    // the weighted mean of DESIGN.md section 7.  Nine sums, so they come back by a copy, not through the mapped payload.
    int resampled = 1;
    if (pf->gated && pf->has_anc)
        if (int rc = slam_resample_happened_host(e, &resampled)) return rc;
    if (!resampled) {
        constexpr int K = kPoseSumsWeighted;
        long long* out = reinterpret_cast<long long*>(pf->res_dev);
        SLAM_HIP_TRY(e, launch_pose_sums(e->stream, x, y, th, idx, pf->n, ref_theta, pf->sums_acc, ticket, out, nullptr, nullptr, 0,
                                         e->carry_buf.as<float>()));
        const void* src = out;
        if (pf->comm) {
            if (int rc = comm_all_gather(pf->comm, pf->res_dev, pf->res_all, K * sizeof(long long))) return rc;
            src = pf->res_all;
        }
        std::vector<long long> all(K * (size_t)pf->world);
        SLAM_HIP_TRY(e, hipMemcpyAsync(all.data(), src, all.size() * 8, hipMemcpyDeviceToHost, e->stream));
        if (int rc = wait_stream(pf)) return rc;
        long long w[K] = { 0 };
        for (int q = 0; q < pf->world; ++q)
            for (int k = 0; k < K; ++k) w[k] += all[K * (size_t)q + k];   // every limb sum of the whole population fits 64 bits
        if (w[8] > 0) {   // (no weight at all: log-weights that are not numbers — the plain mean below)
            double v[4];
            for (int k = 0; k < 4; ++k)   // trunc(sum w16 V / sum w16): C's division truncates
                v[k] = (double)(long long)(((__int128)w[2 * k] * 2097152 + w[2 * k + 1]) / w[8]);
            pose[0] = (float)(v[0] / 4294967296.0);
            pose[1] = (float)(v[1] / 4294967296.0);
            pose[2] = (float)((double)ref_theta + atan2(v[2], v[3]));
            return SLAM_OK;
        }
    }
    long long sums[4] = { 0, 0, 0, 0 };
    if (!pf->comm) {
        const uint32_t seq = ++pf->res_seq;
        SLAM_HIP_TRY(e, launch_pose_sums(e->stream, x, y, th, idx, pf->n, ref_theta, pf->sums_acc, ticket,
                                         reinterpret_cast<long long*>(pf->res_dev), reinterpret_cast<long long*>(pf->d_hres),
                                         reinterpret_cast<uint32_t*>(dev_word(pf, RES_SEQ)), seq));
        if (int rc = wait_result(pf, seq)) return rc;
        memcpy(sums, pf->h_res, sizeof sums);
    } else {   // integer sums: adding the ranks' shares in any order gives the single-GPU bits
        SLAM_HIP_TRY(e, launch_pose_sums(e->stream, x, y, th, idx, pf->n, ref_theta, pf->sums_acc, ticket,
                                         reinterpret_cast<long long*>(pf->res_dev), nullptr, nullptr, 0));
        if (int rc = comm_all_gather(pf->comm, pf->res_dev, pf->res_all, 4 * sizeof(long long))) return rc;
        std::vector<long long> all(4 * (size_t)pf->world);
        SLAM_HIP_TRY(e, hipMemcpyAsync(all.data(), pf->res_all, all.size() * 8, hipMemcpyDeviceToHost, e->stream));
        if (int rc = comm_wait_stream(pf->comm)) return rc;
        for (int q = 0; q < pf->world; ++q)
            for (int k = 0; k < 4; ++k) sums[k] += all[4 * (size_t)q + k];
    }
    const double nt = (double)pf->n_total;
    pose[0] = (float)((double)sums[0] / 4294967296.0 / nt);
    pose[1] = (float)((double)sums[1] / 4294967296.0 / nt);
    pose[2] = (float)((double)ref_theta + atan2((double)sums[2], (double)sums[3]));
    return SLAM_OK;
}

int pf_get_poses_host(slam_pf* pf, float* x, float* y, float* theta)
{
    if (!pf || !x || !y || !theta) return SLAM_ERR_INVALID_ARG;
    const size_t n = (size_t)pf->n;
    float* tmp = pf->pose[1 - pf->cur];   // the other buffer is free between frames
    float* out[3] = { x, y, theta };
    if (pf->comm && pf->has_anc) {   // the ancestors' poses are in the all-gathered array
        if (int rc = comm_all_gather_finish(pf->comm)) return rc;
        for (int k = 0; k < 3; ++k)
            if (int rc = gathered_copy_out(pf, pf->pose_all + k * n, pf->pose_idx[pf->cur], out[k], tmp)) return rc;
        return SLAM_OK;
    }
    const float* p = pf->pose[pf->cur];
    for (int k = 0; k < 3; ++k)
        if (int rc = gathered_copy_out(pf, p + k * n, pf->has_anc ? pf->anc[pf->cur] : nullptr, out[k], tmp)) return rc;
    return SLAM_OK;
}

// dense rows [count][5][Lp] of the particles idx[0 .. count) (nullptr: 0 .. count - 1) of a session on pages, split or split pages
hipError_t rows_of(const slam_pf* pf, const int32_t* idx, int count, float* dense)
{
    hipStream_t s = pf->e->stream;
    const int64_t stride = 5 * (int64_t)pf->Lp;
    if (pf->paged && pf->split) return launch_rows_from_split_pages(s, page_pool(pf), class_store(pf), idx, count, dense, stride, pf->Lp, pf->L);
    if (pf->split) return launch_rows_from_split(s, pf->mean[pf->sp_cur], class_store(pf), idx, count, dense, stride, pf->Lp, pf->L);
    return launch_rows_from_pages(s, page_pool(pf), idx, count, dense, stride, pf->Lp, pf->L);
}

int pf_get_map_host(slam_pf* pf, float* rows)
{
    if (!pf || !rows || !pf->L) return SLAM_ERR_INVALID_ARG;
    const size_t n = (size_t)pf->n, L = (size_t)pf->L, Lp = (size_t)pf->Lp;
    if (pf->comm)
        if (int rc = finish_exchange(pf)) return rc;   // collective: remote ancestors' rows into the staging tail
    if (int rc = settle_means(pf)) return rc;
    const int32_t* idx = pf->has_anc ? pf->anc[pf->cur] : nullptr;   // the pending gather is applied on the way
    float* dense = nullptr;
    const float* src = pf->map[pf->map_cur];
    int rc = SLAM_OK;
    if (pf->paged || pf->split) {   // -> rows in a scratch buffer
        if (hipMalloc((void**)&dense, 5 * Lp * n * 4) != hipSuccess) return SLAM_ERR_HIP;
        if (rows_of(pf, idx, pf->n, dense) != hipSuccess) rc = SLAM_ERR_HIP;
        src = dense;
    } else if (idx) {               // -> the spare row buffer
        rc = slam_gather_map_dev(pf->e, src, pf->map[1 - pf->map_cur], 5 * (int64_t)Lp, 5 * (int64_t)Lp, pf->Lp, pf->Lp, pf->L, idx, pf->n);
        src = pf->map[1 - pf->map_cur];
    }
    if (rc == SLAM_OK) rc = slam_engine_sync(pf->e);
    if (rc == SLAM_OK && hipMemcpy2D(rows, L * 4, src, Lp * 4, L * 4, 5 * n, hipMemcpyDeviceToHost) != hipSuccess) rc = SLAM_ERR_HIP;
    (void)hipFree(dense);
    return rc;
}

int pf_get_map_rows_host(slam_pf* pf, const int32_t* particle, int count, float* rows)
{
    if (!pf || !pf->L || count < 0 || (count > 0 && (!particle || !rows))) return SLAM_ERR_INVALID_ARG;
    for (int k = 0; k < count; ++k)
        if (particle[k] < 0 || particle[k] >= pf->n) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (pf->comm)
        if (int rc = finish_exchange(pf)) return rc;   // collective: remote ancestors' rows into the staging tail
    if (count == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (pf->sel_cap < count) {
        pf->sel_cap = 0;
        if (int rc = replace_scratch(pf, (void**)&pf->sel, 2 * sizeof(int32_t) * (size_t)count, true)) return rc;
        if (!pf->sel) return slam_engine_fail_hip(e, hipErrorOutOfMemory, "particle list");
        pf->sel_cap = count;
    }
    const size_t L = (size_t)pf->L, Lp = (size_t)pf->Lp;
    float* dense = nullptr;
    SLAM_HIP_TRY(e, hipMalloc((void**)&dense, 5 * Lp * (size_t)count * 4));
    int32_t *sel = pf->sel, *src = pf->sel + pf->sel_cap;
    int rc = SLAM_OK;
    auto ok = [&](hipError_t err, const char* what) {
        if (err != hipSuccess && rc == SLAM_OK) rc = slam_engine_fail_hip(e, err, what);
        return err == hipSuccess;
    };
    if (ok(hipMemcpyAsync(sel, particle, sizeof(int32_t) * (size_t)count, hipMemcpyHostToDevice, e->stream), "copy of the particle list") &&
        ok(launch_compose_index(e->stream, sel, pf->has_anc ? pf->anc[pf->cur] : nullptr, count, src), "compose_index")) {
        if (pf->paged || pf->split)
            ok(rows_of(pf, src, count, dense), "rows_of");
        else
            ok(launch_gather_map(e->stream, pf->map[pf->map_cur], dense, 5 * (int64_t)Lp, 5 * (int64_t)Lp, pf->Lp, pf->Lp, pf->L, src,
                                 count), "gather_map");
    }
    if (rc == SLAM_OK) ok(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    if (rc == SLAM_OK) ok(hipMemcpy2D(rows, L * 4, dense, Lp * 4, L * 4, 5 * (size_t)count, hipMemcpyDeviceToHost), "hipMemcpy2D");
    (void)hipFree(dense);
    return rc;
}

}  // namespace

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
    free_page_tables(pf);
    free_split_tables(pf);
    for (void* p : { (void*)pf->score, (void*)pf->logw, (void*)pf->count, (void*)pf->first, (void*)pf->pose_all, (void*)pf->pose_stage, (void*)pf->first_all,
                     (void*)pf->d_sum, (void*)pf->totals, (void*)pf->d_plan, (void*)pf->sbuf,
                     (void*)pf->rbuf, (void*)pf->res_dev, (void*)pf->sums_acc, pf->res_all })
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
        if (pf->paged)   // split pages: every particle names ONE shared page of zero means, the rest of the pool is free
            SLAM_HIP_TRY(pf->e, launch_pages_reset(pf->e->stream, page_pool(pf), (int64_t)pf->n * pf->nb));
        if (int rc = slam_engine_sync(pf->e)) return rc;
    } else if (pf->paged) {   // every particle names ONE shared page of landmarks not seen yet
        SLAM_HIP_TRY(pf->e, launch_pages_reset(pf->e->stream, page_pool(pf), (int64_t)pf->n * pf->nb));
        if (int rc = slam_engine_sync(pf->e)) return rc;
    } else if (pf->L) {   // P_xx = -1: "not seen yet"
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
    if (indirect && hipMalloc((void**)&dense, 5 * (size_t)pf->Lp * pf->n * 4) != hipSuccess) return SLAM_ERR_HIP;
    int rc = SLAM_OK;
    if (hipMemcpy2D(dense, (size_t)pf->Lp * 4, rows, (size_t)pf->L * 4, (size_t)pf->L * 4, 5 * (size_t)pf->n,
                    hipMemcpyHostToDevice) != hipSuccess)
        rc = SLAM_ERR_HIP;
    if (indirect) {
        if (rc == SLAM_OK) rc = slam_pf_set_map_dev(pf, dense, 5 * (int64_t)pf->Lp, pf->Lp);
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
        SLAM_HIP_TRY(e, hipMemcpy2DAsync(pf->map[pf->map_cur] + (size_t)pl * pf->Lp, 5 * (size_t)pf->Lp * 4,
                                         d_rows + (size_t)pl * plane_stride, (size_t)row_stride * 4, (size_t)pf->L * 4,
                                         (size_t)pf->n, hipMemcpyDeviceToDevice, e->stream));
    return evidence_from_maps(pf);   // (pruning: the loaded maps are trusted)
}

int slam_pf_is_paged(const slam_pf* pf) { return pf && pf->paged ? 1 : 0; }

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
    const bool iso = meas_cov[0] == pf->cfg.meas_var && meas_cov[1] == 0.0f && meas_cov[2] == pf->cfg.meas_var;
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
        pf->prune_on = false;
        pf->detect_on = false;
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
        const size_t tab = ((size_t)pf->n * (size_t)pf->Lp + 15) & ~(size_t)15, st = (size_t)pf->n * 3 * sizeof(int32_t);
        SLAM_HIP_TRY(e, dev_alloc((void**)&pf->assoc_tab, tab + st));   // one allocation: the table, then the stats
        pf->assoc_stats = reinterpret_cast<int32_t*>(pf->assoc_tab + tab);
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->assoc_tab, SLAM_ASSOC_NONE, tab, e->stream));
        SLAM_HIP_TRY(e, hipMemsetAsync(pf->assoc_stats, 0, st, e->stream));
    }
    pf->assoc_on = true;
    pf->assoc_aniso = false;   // (slam_pf_assoc_cov_set behind this call says otherwise)
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
    const bool iso = meas_cov[0] == pf->cfg.meas_var && meas_cov[1] == 0.0f && meas_cov[2] == pf->cfg.meas_var;
    for (int k = 0; k < 3; ++k) pf->assoc_cov[k] = meas_cov[k];
    pf->assoc_aniso = !iso;
    return SLAM_OK;
}

int slam_pf_assoc_device_view(slam_pf* pf, const uint8_t** assoc, int32_t* assoc_stride, const int32_t** stats)
{
    if (!pf || !assoc || !assoc_stride || !stats) return SLAM_ERR_INVALID_ARG;
    if (!pf->assoc_tab) return SLAM_ERR_NOT_READY;   // slam_pf_assoc_set never switched association on
    *assoc = pf->assoc_tab;
    *assoc_stride = pf->Lp;
    *stats = pf->assoc_stats;
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
        const size_t buf = ((size_t)pf->n * (size_t)pf->Lp + 15) & ~(size_t)15, st = (size_t)pf->n * 2 * sizeof(int32_t);
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

int slam_pf_detect_set(slam_pf* pf, const slam_detect_params* params)
{
    if (!pf) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (!params) {   // off: the session runs exactly what it ran before the first call
        pf->detect_on = false;
        return SLAM_OK;
    }
    if (!pf->assoc_on) {   // (which is what every layout but rows, a sharded session and a 2x2 covariance come down to)
        snprintf(e->err, sizeof e->err, "the detector makes the detections the association reads: it needs data association switched "
                                        "on (slam_pf_assoc_set: the row layout on one GPU, not sharded, meas_var * I)");
        return SLAM_ERR_INVALID_ARG;
    }
    if (!slam_detect_params_ok(params)) {
        slam_detect_params_error(e);
        return SLAM_ERR_INVALID_ARG;
    }
    pf->detect_on = true;
    pf->detect_params = *params;
    return SLAM_OK;
}

int slam_pf_evidence_device_view(slam_pf* pf, const uint8_t** ev, int32_t* ev_stride, const int32_t** stats)
{
    if (!pf || !ev || !ev_stride || !stats) return SLAM_ERR_INVALID_ARG;
    if (!pf->ev[0]) return SLAM_ERR_NOT_READY;   // slam_pf_prune_set never switched pruning on
    *ev = pf->ev[pf->map_cur];
    *ev_stride = pf->Lp;
    *stats = pf->ev_stats;
    return SLAM_OK;
}

int slam_pf_get_evidence_host(slam_pf* pf, uint8_t* ev)
{
    if (!pf || !ev) return SLAM_ERR_INVALID_ARG;
    if (!pf->ev[0]) return SLAM_ERR_NOT_READY;
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    const uint8_t* src = pf->ev[pf->map_cur];
    if (pf->has_anc) {   // the pending gather is applied on the way, into the spare buffer
        if (int rc = slam_evidence_gather_dev(e, src, pf->ev[1 - pf->map_cur], pf->Lp, pf->anc[pf->cur], pf->n)) return rc;
        src = pf->ev[1 - pf->map_cur];
    }
    if (int rc = slam_engine_sync(e)) return rc;
    SLAM_HIP_TRY(e, hipMemcpy2D(ev, (size_t)pf->L, src, (size_t)pf->Lp, (size_t)pf->L, (size_t)pf->n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_pf_rows_received(const slam_pf* pf) { return pf ? pf->rows_received : 0; }
int64_t slam_pf_frames_resampled(const slam_pf* pf) { return pf ? pf->frames_resampled : 0; }
int64_t slam_pf_layout_changes(const slam_pf* pf) { return pf ? pf->conversions : 0; }

int slam_pf_device_view(slam_pf* pf, slam_pf_view* out)
{
    if (!pf || !out) return SLAM_ERR_INVALID_ARG;
    if (int rc = settle_means(pf)) return rc;
    out->pose = pf->pose[pf->cur];
    const bool rows = pf->L && !pf->paged && !pf->split;   // pages and split maps have no rows to look at: slam_pf_set_map_dev
    out->map = rows ? pf->map[pf->map_cur] : nullptr;
    out->map_spare = rows ? pf->map[1 - pf->map_cur] : nullptr;
    out->anc = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    out->row_stride = 5 * (int64_t)pf->Lp;
    out->plane_stride = pf->Lp;
    out->map_rows = pf->cap;
    out->score = pf->has_anc ? pf->score : nullptr;
    out->logw = pf->has_anc ? pf->logw : nullptr;
    out->loglik = pf->has_anc && pf->last_ekf && pf->e->ll_n == pf->n ? pf->e->ll_buf.as<float>() : nullptr;
    out->count = pf->has_anc ? pf->count : nullptr;
    return SLAM_OK;
}

int slam_pf_layout(const slam_pf* pf)
{
    if (!pf || !pf->L) return SLAM_MAP_ROWS;
    return pf->paged ? (pf->split ? SLAM_MAP_SPLIT_PAGES : SLAM_MAP_PAGES) : pf->split ? SLAM_MAP_SPLIT : SLAM_MAP_ROWS;
}

int slam_pf_split_device_view(slam_pf* pf, slam_pf_split_view* out)
{
    if (!pf || !out) return SLAM_ERR_INVALID_ARG;
    if (!pf->split || !pf->L) return SLAM_ERR_NOT_READY;
    if (int rc = settle_means(pf)) return rc;
    out->mean = pf->paged ? nullptr : pf->mean[pf->sp_cur];   // split pages: the means are on pages (slam_pf_paged_device_view)
    out->cov = pf->cov;
    out->cls = pf->cls[pf->sp_cur];
    out->live = pf->live[pf->live_cur];
    out->live_count = pf->cov_cnt + pf->cov_phase;
    out->plane_stride = pf->Lp;
    out->rows = pf->cap;
    return SLAM_OK;
}

int slam_pf_split_covx_view(slam_pf* pf, const float** covx)
{
    if (!pf || !covx) return SLAM_ERR_INVALID_ARG;
    if (!pf->split || !pf->L) return SLAM_ERR_NOT_READY;
    *covx = pf->covx;
    return SLAM_OK;
}

int slam_pf_paged_device_view(slam_pf* pf, slam_pf_paged_view* out)
{
    if (!pf || !out) return SLAM_ERR_INVALID_ARG;
    if (!pf->paged) return SLAM_ERR_NOT_READY;
    if (int rc = settle_means(pf)) return rc;
    const PageGeom g = pf->split ? split_geom(pf) : PageGeom();
    out->pool = pf->split ? split_pool(pf) : pf->pool;
    out->planes = g.planes;
    out->reserved = 0;
    out->half_pages = pf->split ? g.half_pages : (int64_t)pf->npages;
    out->gap_floats = g.gap;
    out->table = pf->pt[pf->pt_cur];
    out->freelist = pf->freelist;
    out->state = pf->page_scratch;
    out->stamp = pf->stamp;
    out->stamp_now = pf->stamp_now;
    out->page_landmarks = kPageLandmarks;
    out->pages_per_particle = pf->nb;
    out->table_rows = pf->cap;
    out->npages = pf->npages;
    return SLAM_OK;
}

int slam_pf_best(slam_pf* pf, float pose[3], float* logw, int32_t* index) { return collective_result(pf, pf_best(pf, pose, logw, index)); }
int slam_pf_mean(slam_pf* pf, float ref_theta, float pose[3]) { return collective_result(pf, pf_mean(pf, ref_theta, pose)); }
int slam_pf_get_poses_host(slam_pf* pf, float* x, float* y, float* theta) { return collective_result(pf, pf_get_poses_host(pf, x, y, theta)); }
int slam_pf_get_map_host(slam_pf* pf, float* rows) { return collective_result(pf, pf_get_map_host(pf, rows)); }
int slam_pf_get_map_rows_host(slam_pf* pf, const int32_t* particle, int count, float* rows) { return collective_result(pf, pf_get_map_rows_host(pf, particle, count, rows)); }
}  // extern "C"
