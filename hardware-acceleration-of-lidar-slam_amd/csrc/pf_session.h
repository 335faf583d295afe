// pf_session.h — internal to the four units of the slam_pf_* session of include/slam_hip.h (device buffers + one whole frame
// per call, for a plain C host): pf_session.hip (the object and its switches), pf_session_store.hip (the map storage forms),
// pf_session_frame.hip (one frame) and pf_session_read.hip (what a host reads back).  The object, the words of its result block,
// the facts of a frame and the functions that cross the units' boundaries; nothing else includes it.
// One GPU (slam_pf_create) or one rank of a population sharded over several GPUs (slam_pf_create_sharded): the frame is built
// on the public stage entry points either way, and in the sharded form every exchange step between the ranks is issued from
// the session through comm.h (RCCL over xGMI, or the in-process transport) — nothing but these units sits between the launches.
// The landmark maps are kept as rows, pages, split (means per particle, covariances per class) or split pages; a
// SLAM_MAP_AUTO session lives on split and moves its means onto pages and back while it runs (auto_layout).
// No counterpart in the reference; specification: oracle/slam_oracle_pf.c; the shape
// "handle created once in main and threaded through" is the reference's (Hadrware_acclereated.cpp:842-845, 284).
#pragma once

#include <hip/hip_runtime.h>

#include "comm.h"
#include "engine_internal.h"
#include "kernels.h"

// The words of the engine's mapped result block (slam_pf::h_res as the host sees it, d_hres as the device does)
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
    RES_MOMENTS = 32,     // 32..71: kPoseMoments x 8 bytes, what slam_pf_spread asks for (behind RES_SEQ as well)
    RES_RESEED = 72,      // 72..73 {replaced, chosen but not replaced} of slam_pf_known_map_reseed (behind RES_SEQ as well)
    RES_RESEED_PAIRS = 74,   // 74..77 {replaced, j1 empty, too close, no partner} of slam_pf_known_map_reseed_pairs (behind RES_SEQ as well)
    RES_MODES = 128,      // 128..247: kModesWords x 8 bytes, what slam_pf_modes asks for (behind RES_SEQ as well)
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
    float* res_dev = nullptr;       // device copy of the payload (what the ranks all-gather): kResBytes
    unsigned long long* sums_acc = nullptr;   // 9 accumulators + ticket of pose_sums_kernel (kept zeroed by the kernel)
    unsigned long long* moments_acc = nullptr;   // kPoseMoments accumulators + ticket of pose_moments_kernel (likewise)
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
    bool split = false;             // (set when the session is made and never cleared: AUTO moves between split and split pages)
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
    // slam_pf_assoc_detcov_set: association under the covariance each detection carries — the same two launches under it
    // (update_noise); cleared by slam_pf_assoc_set and slam_pf_assoc_cov_set
    bool assoc_detcov = false;
    // slam_pf_detect_noise_set: the detector's launch runs the noise model (slam_detect_scan_noise_dev), so its detections carry
    // covariances; cleared by slam_pf_detect_set, slam_pf_detect_fit_set and slam_pf_assoc_set(0)
    bool detect_noise_on = false;
    slam_detect_noise detect_noise = { 0.0f, 0.0f, 0.0f };
    uint8_t* assoc_tab = nullptr;     // [n][Lp] the last frame's table, indexed like `score`; made by the first slam_pf_assoc_set
    int32_t* assoc_stats = nullptr;   // [n][3], behind the table in the same allocation
    // slam_pf_prune_set (only while association is on): one evidence byte per (particle, landmark slot) beside the rows, brought up
    // to date behind every associating update (slam_landmark_evidence_dev); ev[map_cur] belongs to map[map_cur] — the two flip together
    bool prune_on = false;
    int prune_hit = 0, prune_miss = 0, prune_cmax = 0;
    float prune_range = 0.0f;
    uint8_t* ev[2] = { nullptr, nullptr };   // [n][Lp] each, one allocation made by the first slam_pf_prune_set that switches on
    int32_t* ev_stats = nullptr;             // [n][2] pruned, seen after pruning (the last frame that ran the stage), behind them
    // slam_pf_prune_sight_set (only while association is on; in force only while pruning is): the evidence stage of an observing
    // frame is slam_landmark_evidence_sight_dev behind one slam_sight_table_dev over the engine's scan — the same buffers and stats
    int sight_bins = 0;                      // 0: off
    float sight_margin = 0.0f;
    int32_t* sight_spared = nullptr;         // [n] landmarks spared a miss (the last frame that ran the sight stage); made at the first switch-on
    // slam_pf_prune_fov_set (accepted and in force as line of sight is): the evidence stage of an observing frame is
    // slam_landmark_evidence_fov_dev — behind the sight table and with use_sight = 1 where sight_bins != 0
    bool fov_on = false;
    float fov_lo = 0.0f, fov_hi = 4.0f;      // slam_fov_bound(angle_min + edge), slam_fov_bound(angle_max - edge)
    int32_t* fov_outside = nullptr;          // [n] landmarks due a miss outside the arc (the last frame that ran the stage); made at the first switch-on
    // slam_pf_merge_set (only while association is on): behind the update and the evidence stage of every observing frame,
    // slam_landmark_merge_dev on the row (and, while pruning is on, the evidence buffer) that frame wrote
    float merge_gate = 0.0f;                 // 0: off
    int32_t* merge_stats = nullptr;          // [n][3] merged, refused, seen after (the last frame that ran the stage); made at the first switch-on
    // slam_pf_assoc_weight_set (only while association is on): the evidence stage of every observing frame also counts its misses,
    // and slam_assoc_weight_dev runs behind the merge, in front of the weights, on the engine's log-likelihood buffer
    bool assoc_weight_on = false;
    float assoc_weight_log[3] = { 0.0f, 0.0f, 0.0f };   // log_new, log_clutter, log_miss
    int32_t* assoc_weight_missed = nullptr;  // [n] the frame's misses, then (float) [n] the terms that were added; made at the first switch-on
    float* assoc_weight_terms = nullptr;     // (behind the misses in the same allocation)
    // slam_pf_detect_set (only while association is on): every observing frame makes its detections from the engine's scan
    // (slam_detect_scan_dev), issued in front of the frame's first launch
    bool detect_on = false;
    slam_detect_params detect_params{};
    // slam_pf_detect_fit_set: the detector's launch runs the fit (slam_detect_scan_fit_dev); cleared by slam_pf_detect_set and
    // slam_pf_assoc_set(0)
    bool detect_fit_on = false;
    slam_detect_fit detect_fit{};
    // slam_pf_known_map_set (n_landmarks == 0, one GPU): every observing frame associates its detections with ONE known map all
    // particles share (slam_localise_dev on the prepared map, then the clutter term) and weighs with the result; no map is kept
    // per particle and none is changed.  The detector switches are accepted while it is on.
    bool known_on = false;
    bool known_detcov = false;        // slam_pf_known_map_detcov_set: the stage under the detections' own covariances, on the map as given
    bool known_ll = false;            // the engine's log-likelihood buffer was last claimed by this mode
    int known_L = 0, known_Lp = 0;    // landmarks; plane stride of the prepared map (known_L rounded up to 32)
    size_t known_cap = 0;             // floats of the allocation behind known_prep
    float known_gate = 0.0f, known_log_clutter = 0.0f;
    float* known_prep = nullptr;      // [6][known_Lp] the prepared map, then [5][known_Lp] the map as it was given
    int32_t* known_stats = nullptr;   // [n][3] matched, 0, dropped (the last frame that ran the stage); an allocation of its own
    // slam_pf_known_map_miss_set (only while a known map is set): the stage of every observing frame is its miss form — behind one
    // slam_sight_table_dev where line of sight is on — and slam_assoc_weight_dev charges log_miss per landmark it counted as missed
    bool known_miss_on = false;
    float known_log_miss = 0.0f;
    slam_localise_view known_view{};  // view_range, the arc (0, 4: the whole circle), sight != 0 and its margin
    int known_sight_bins = 0;         // 0: no line of sight
    int32_t* known_missed = nullptr;  // [3][n] missed, spared, outside (the last frame that ran the miss form); made at the first switch-on
    // slam_pf_known_map_reseed: from a successful reseed until the next step the last frame's log-weights belong to no pose
    // (slam_pf_best is refused)
    bool reseeded = false;
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

    // floats from one particle's row to the next
    int64_t row_stride() const { return 5 * (int64_t)Lp; }    // map[]: x, y, Pxx, Pxy, Pyy
    int64_t mean_stride() const { return 2 * (int64_t)Lp; }   // mean[] and covx
    int64_t cov_stride() const { return 3 * (int64_t)Lp; }
    // bytes of one byte per (particle, landmark slot), rounded up to 16: what lies behind such a table stays aligned
    size_t byte_table() const { return ((size_t)n * (size_t)Lp + 15) & ~(size_t)15; }
    // is a 2x2 covariance {xx, xy, yy} just meas_var * I?  (then the session's own isotropic kernels run: the same bits)
    bool is_meas_var(const float q[3]) const { return q[0] == cfg.meas_var && q[1] == 0.0f && q[2] == cfg.meas_var; }
};

namespace slam::session {

constexpr size_t kResBytes = 256;   // of res_dev and of each rank's share of res_all: the largest payload is kPoseMoments x 8 bytes

inline hipError_t dev_alloc(void** p, size_t bytes) { return hipMalloc(p, bytes ? bytes : 4); }

// a word of the mapped result block as the host / the device sees it
inline int32_t* host_word(const slam_pf* pf, ResWord w) { return reinterpret_cast<int32_t*>(pf->h_res) + w; }
inline int32_t* dev_word(const slam_pf* pf, ResWord w) { return reinterpret_cast<int32_t*>(pf->d_hres) + w; }

inline int wait_stream(slam_pf* pf)
{
    if (pf->comm) return comm_wait_stream(pf->comm);
    SLAM_HIP_TRY(pf->e, hipStreamSynchronize(pf->e->stream));
    return SLAM_OK;
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
    bool localise;       // a known map is set and the host asks for observations: the frame weighs with the localise stage (no maps: ekf is false)
};

// ---- pf_session_store.hip: the storage forms and the moves between them
bool alloc_store(slam_pf* pf);
bool alloc_page_tables(slam_pf* pf);
void free_page_tables(slam_pf* pf);
bool alloc_split_tables(slam_pf* pf);
void free_split_tables(slam_pf* pf);
void place_split(slam_pf* pf, int base);
float* split_pool(const slam_pf* pf);
PageGeom split_geom(const slam_pf* pf);
PagePool page_pool(const slam_pf* pf);
ClassStore class_store(const slam_pf* pf);
void split_new_epoch(slam_pf* pf);
int split_from_rows(slam_pf* pf, const float* d_rows, int64_t row_stride, int plane_stride, int nrows);
int split_means_to_pages(slam_pf* pf);
int auto_layout(slam_pf* pf);
int replace_scratch(slam_pf* pf, void** buf, size_t bytes, bool drain_always);
int grow(slam_pf* pf, float** buf, size_t* have, size_t want);
bool survivor_buffers(slam_pf* pf);
int materialise(slam_pf* pf, bool filtered);
int settle_means(slam_pf* pf);
// ---- pf_session_frame.hip: what the read-backs share with the frame
int ancestor_poses(slam_pf* pf, const float** base, const int32_t** idx);
int finish_exchange(slam_pf* pf);

}  // namespace slam::session
