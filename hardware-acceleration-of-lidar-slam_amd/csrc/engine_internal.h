// engine_internal.h — the engine object shared by the translation units that implement the C ABI
// (engine.hip and the engine_*.hip units by stage — match, ekf, assoc, evidence, merge, resample —, the pf_session*.hip units, comm.hip, mapper.hip).  Not part of the public interface.
#pragma once

#include <hip/hip_runtime.h>
#include <stdio.h>

#include <vector>

#include "estimate_host.h"
#include "kernels.h"

using slam::EventPair;

struct slam_comm;

namespace slam_detail {

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes)
    {
        if (bytes <= cap) return hipSuccess;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 256;
        hipError_t err = hipMalloc(&p, want);
        if (err == hipSuccess) cap = want;
        return err;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

struct GridSlot {
    bool ready = false;
    slam_grid_meta meta{};
    const float* d_edt = nullptr;   // owned (edt_buf) or adopted
    DevBuf occ_buf, edt_buf;
    // the byte-per-cell copy the many-pose scorers gather from (kernels.h: ScoreGrid::packed), made on the first such call
    // after the grid changed: 0 = not made yet, 1 = in use, 2 = this grid has no such copy (values the table cannot give back)
    int packed_state = 0;
    DevBuf packed_buf, table_buf;   // table_buf: 256 floats + the two flag words of launch_edt_pack
};

constexpr int kLattice = 27;
// device/host staging layout of one FastMatch call (floats):
//   in : X[27] Y[27] CT[27] ST[27] LAST[4]
//   out: SCORE[27] COUNT[27] NLAST[1] HITS[SLAM_MAX_BEAMS]
constexpr int kFmIn = 4 * kLattice + 4;
constexpr int kFmOut = 2 * kLattice + 1 + SLAM_MAX_BEAMS;
// the chained pair of FastMatch calls (slam_engine_fastmatch_pair), behind the arrival flag's 4 words: in — the nine headings of
// the second call's lattices as cos[9] | sin[9], its step, a spare word; out — the first call's scores and counts
constexpr int kFmPairIn = 20;
constexpr int kFmPair = kFmPairIn + 2 * kLattice;
constexpr unsigned kStageSlots = 8;
constexpr size_t kStageFloats = 3 * SLAM_MAX_OBS > 2 * SLAM_MAX_BEAMS ? 3 * SLAM_MAX_OBS : 2 * SLAM_MAX_BEAMS;

}  // namespace slam_detail

using namespace slam_detail;

struct slam_engine {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    char err[512] = { 0 };

    GridSlot grid[SLAM_MAX_GRID_SLOTS];

    const float *d_bx = nullptr, *d_by = nullptr;   // owned (scan_buf) or adopted
    int nbeams = -1;
    DevBuf scan_buf;

    // observations of the current frame as a table indexed by landmark (zx NaN = not observed)
    DevBuf obs_buf;   // zx[L] zy[L] when uploaded from the host
    int obs_nlandmarks = -1;
    const float *d_obs_zx = nullptr, *d_obs_zy = nullptr;

    // detections of the current frame: sensor-frame points without identity (slam_detections_upload_host / _set_dev), what
    // slam_associate_dev and slam_ekf_update_assoc_dev read
    DevBuf det_buf;   // zx[SLAM_MAX_DETECTIONS] zy[SLAM_MAX_DETECTIONS] when uploaded from the host
    int ndet = -1;
    const float *d_det_zx = nullptr, *d_det_zy = nullptr;
    int64_t assoc_launches[2] = { 0, 0 };   // slam_assoc_counts: associate launches, assoc-update launches (in no form counter)
    int64_t assoc_aniso_launches[2] = { 0, 0 };   // slam_assoc_aniso_counts: the same two under a 2x2 Q (in no other counter)
    // ... and, optionally, a covariance per detection beside them (slam_detections_cov_upload_host / _set_dev): what
    // slam_associate_detcov_dev and slam_ekf_update_assoc_detcov_dev read.  Whatever installs new detections drops it.
    DevBuf detcov_buf;   // qxx[SLAM_MAX_DETECTIONS] qxy[..] qyy[..] when uploaded from the host
    const float *d_det_qxx = nullptr, *d_det_qxy = nullptr, *d_det_qyy = nullptr;
    bool det_has_cov = false;
    int64_t assoc_detcov_launches[2] = { 0, 0 };   // slam_assoc_detcov_counts: the same two under per-detection Q (in no other counter)
    int64_t evidence_launches[2] = { 0, 0 };   // slam_evidence_counts: evidence launches, init launches (in no other counter)
    // the sight table of the current scan (slam_sight_table_dev), what the evidence stage reads with line of sight; whatever hands a
    // scan over drops it (sight_bins = 0), so a stale table is never read
    DevBuf sight_buf;   // kSightMaxBins floats
    int sight_bins = 0;
    int64_t sight_launches[2] = { 0, 0 };   // slam_sight_counts: table launches, stage launches (in no other counter)
    int64_t fov_launches = 0;               // slam_fov_counts: launches of the stage with a field of view (in no other counter)
    int64_t merge_launches = 0;             // slam_merge_count: launches of the merge stage (in no other counter)
    int64_t assoc_weight_launches = 0;      // slam_assoc_weight_count: launches of slam_assoc_weight_dev (in no other counter)
    int64_t localise_launches[2] = { 0, 0 };   // slam_localise_counts: prepare launches, stage launches (in no other counter)
    int64_t localise_detcov_launches = 0;      // slam_localise_detcov_count: stage launches under per-detection Q (in no other counter)
    int64_t localise_miss_launches = 0;        // slam_localise_miss_count: launches of the miss form, either noise (in no other counter)
    int64_t reseed_launches = 0;               // slam_pose_reseed_count: launches of slam_pose_reseed_dev (in no other counter)
    DevBuf reseed_buf;                         // its two accumulators and ticket (kept zeroed), then the two counts
    int64_t reseed_pair_launches = 0;          // slam_pose_reseed_pairs_count: launches of slam_pose_reseed_pairs_dev (in no other counter)
    DevBuf reseed_pair_buf;                    // its four accumulators and ticket (kept zeroed), then the four counts
    // the detector (slam_detect_scan_dev): its kernel writes det_buf and leaves {ndet, sequence} in mapped host memory; until the
    // next stage that needs the count on the host has picked it up (slam_engine_resolve_detections) it is PENDING
    int32_t* h_det = nullptr;
    int32_t* d_hdet = nullptr;
    uint32_t det_seq = 0;
    bool det_pending = false;
    bool det_from_scan = false;   // the current detections are the detector's: det_buf holds 0 from ndet on
    int64_t detect_launches = 0;   // slam_detect_count (in no other counter)
    int64_t detect_fit_launches = 0;   // slam_detect_fit_count: those of them that ran the fit
    int64_t detect_noise_launches = 0;   // slam_detect_noise_count: those of them that ran the noise model

    DevBuf fm_buf;             // kFmIn + kFmOut floats
    DevBuf fm_work;            // 2 x 27 x SLAM_MAX_BEAMS floats: per-candidate hit rows of the lattice kernel, two sweeps (the chained pair)
    float* h_fm = nullptr;     // pinned + mapped: lattice candidates in, results out, then one uint32 arrival flag
    float* d_hfm = nullptr;    // the same memory as the device sees it (zero-copy FastMatch I/O)
    uint32_t fm_seq = 0;
    int32_t* h_plan = nullptr;   // pinned + mapped: exchange plan of the last slam_ancestors_sharded_dev, then one arrival flag
    int32_t* d_hplan = nullptr;
    uint32_t plan_seq = 0;
    int plan_world = 0;
    int exch_cap = 0x7fffffff;   // staging rows a rank can take in one exchange (slam_exchange_set_capacity)
    DevBuf scratch;            // per-call temporaries of the *_dev stages
    DevBuf bmax_buf;           // block maxima left by slam_logweight_dev (read by slam_quantise_scan_dev)
    int bmax_count = 0, bmax_n = -1;
    DevBuf scan_state;         // tile-local CDF u64[n] + tile totals, left by slam_quantise_scan_dev
    int scan_n = -1;
    DevBuf shard_buf;          // flag scans of the last slam_ancestors_sharded_dev call (read by slam_migrate_pack_dev)
    int shard_n = -1;
    DevBuf first_buf;          // scratch `first` array of slam_ancestors_from_scan_dev's large-n fallback
    DevBuf ll_buf;             // log-likelihood [n] of the last EKF call
    int ll_n = -1;
    // resample gate (slam_resample_gate_set): threshold, the device flag "the last resample stage did resample", the
    // same verdict in mapped host memory {int32 resampled, uint32 sequence}, and the weights carried over a frame
    // that did not resample
    uint32_t gate_frac_q16 = 0;
    DevBuf gate_buf;           // int32 flag
    int32_t* h_gate = nullptr;
    int32_t* d_hgate = nullptr;
    uint32_t gate_seq = 0;
    DevBuf carry_buf;          // float[n]
    int carry_n = -1;
    DevBuf spread_buf;         // slam_pose_spread_dev: the accumulators and tickets of the two launches (kept zeroed), then their sums
    DevBuf modes_buf;          // slam_pose_modes_dev / slam_pf_modes: the table, the list of claimed slots, the control words (all kept zeroed), the result; made by the first call
    bool modes_clean = false;  // ... and every launch so far left it zeroed (a failed launch: cleared again before the next)
    int modes_cus = 0;         // compute units of the device (asked once)

    // feedback of the resample stages: roughly how many distinct ancestors the last one left {count, n} (mapped host
    // memory, read without synchronisation: it only steers the choice between two equivalent EKF kernels)
    int32_t* h_heads = nullptr;
    int32_t* d_hheads = nullptr;
    DevBuf heads_buf;          // {count, ticket}

    slam::HeadsOut heads_out()
    {
        slam::HeadsOut h;
        h.counter = heads_buf.as<unsigned int>();
        h.h_out = d_hheads;
        return h;
    }
    // in-place updates (frames that keep their population) have two equivalent kernels as well: whole rows in batches of
    // 128 landmarks, or only the observed landmarks from a compact list (obs_list: ids | zx | zy | rounds, [L] each, then
    // {nobs, highest round}).  The list is built at most once per observation table; {nobs, L} of the last build sit in
    // mapped host memory and steer the choice for the following frames (read without synchronisation).
    DevBuf obs_list;
    bool obs_list_valid = false;
    bool obs_table_owned = false;   // the table is the engine's own copy (slam_obs_upload_host), not the caller's arrays
    int32_t* h_obs = nullptr;
    int32_t* d_hobs = nullptr;
    // 1024 bytes of mapped host memory the engine's (one) particle-filter session delivers its results through (pf_session.h: ResWord).  It belongs to
    // the ENGINE, not to the session: freeing pinned host memory makes the driver hold the process's queues for 65-80 ms some
    // 10-50 ms later (profiles/r03_stall_trigger.txt) — a session that came and went would stall the frames of the next one.
    void* h_block = nullptr;        // the one pinned allocation every h_* pointer of the engine points into
    void* h_pf_res = nullptr;
    void* d_hpf_res = nullptr;
    bool frame_fusion = true;       // slam_frame_fusion_set
    bool survivor_rows = true;      // slam_survivor_rows_set
    int64_t front_launches = 0;
    int32_t front_last[2] = { 0, 0 };   // slam_frame_front_last: particles per updating wavefront, lanes per pose
    int ekf_inplace_form = -1;   // slam_ekf_inplace_form_set: -1 by the feedback, 0 whole rows, 1 observed landmarks only
    int64_t ekf_inplace_launches[2] = { 0, 0 };
    slam_comm* comm = nullptr; // the communicator made on this engine, if any: host-side waits poll it for failures
    int live_sessions = 0;     // slam_pf sessions alive on this engine (at most one: the stages keep per-population state here)
    bool pf_paged = false;     // slam_pf_paged_set: sessions made from now on keep their maps as copy-on-write pages
    int ekf_form = -1;         // slam_ekf_form_set: -1 choose by the feedback, 0 row per wavefront, 1 / 2 grouped by 4 / 2
    int64_t ekf_form_launches[2] = { 0, 0 };   // out-of-place launches so far: [0] one wavefront per particle, [1] grouped
    int64_t ekf_aniso_launches = 0;            // slam_ekf_update_aniso_dev launches so far (they count in neither form counter)
    // particles per wavefront of an out-of-place update that gathers through `anc` (0 = one wavefront per particle).  With the
    // covariance part of the update hoisted (ekf_prepare) the kernel is memory-bound and behaves like the grouped pure copy of
    // profiles/copy_ceiling.hip: 2 rows per wavefront beat 4 and 8 (update alone at 64k x 500: 133 | 145 | 155 us; fused
    // front at 512k x 5000: 8.10 against 9.00 ms, at 64k x 2000: 0.558 against 0.578 ms per frame) — except in the fused
    // front of a small frame, where 4 keep the number of updating workgroups per scoring workgroup low (64k x 500: 143
    // against 160 us; 3 particles per wavefront: 143.5 against 142.6 us fused, 138 against 134 us alone) as long as neighbours
    // share ancestors (fewer than 3 distinct in 10 slots, as far as the last resample stage reported).
    // Split layout: the kernel is bound by its vector instructions and by what a wavefront does once per pass whatever its
    // group (observation flags, the class's covariances, its own start-up with the motion sample), so larger groups win:
    // fused front at 64k x 500: 2 particles per wavefront 116 us, 4: 99 us, 8: 92.6 us.
    int ekf_group_size(int n, bool has_anc, int plane_stride, bool fused, bool split = false) const
    {
        if (ekf_form >= 0) return ekf_form == 0 ? (split ? 2 : 0) : (ekf_form == 2 ? 2 : 4);
        if (split) {
            const int heads = h_heads[0], hn = h_heads[1];
            return hn == n && (int64_t)heads * 10 < (int64_t)n * 3 ? 8 : 4;
        }
        if (!has_anc) return 0;
        if (!fused) return 2;
        const int heads = h_heads[0], hn = h_heads[1];
        const bool few_distinct = hn == n && (int64_t)heads * 10 < (int64_t)n * 3;
        return few_distinct && (int64_t)n * plane_stride < (int64_t)1 << 26 ? 4 : 2;
    }

    slam::GateOut gate_next()
    {
        slam::GateOut g;
        g.d_flag = gate_buf.as<int32_t>();
        g.h_flag = d_hgate;
        g.seq = ++gate_seq;
        return g;
    }
    // pinned staging ring for the per-frame sensor uploads: one host-to-device copy per upload, and the
    // host only waits if kStageSlots uploads are still in flight
    float* h_stage = nullptr;
    hipEvent_t stage_ev[kStageSlots] = {};
    unsigned stage_next = 0;

    float* stage_acquire()
    {
        const unsigned k = stage_next++ % kStageSlots;
        if (stage_ev[k]) (void)hipEventSynchronize(stage_ev[k]);
        return h_stage + (size_t)k * kStageFloats;
    }
    hipError_t stage_release(const float* slot)
    {
        const unsigned k = (unsigned)((slot - h_stage) / kStageFloats);
        if (!stage_ev[k]) {
            hipError_t err = hipEventCreateWithFlags(&stage_ev[k], hipEventDisableTiming);
            if (err != hipSuccess) return err;
        }
        return hipEventRecord(stage_ev[k], stream);
    }
    DevBuf host_io[6];         // temporaries of the *_host convenience calls

    // per-kernel HIP-event timing (slam_profile_*)
    int prof_mask = 0;
    std::vector<EventPair> prof_pool[SLAM_PROF_COUNT];   // grown on demand, reused after each read
    size_t prof_used[SLAM_PROF_COUNT] = {};
    EventPair prof_cur{};

    const EventPair* prof_next(int k)
    {
        if (!(prof_mask & (1 << k))) return nullptr;
        auto& pool = prof_pool[k];
        if (prof_used[k] == pool.size()) {
            EventPair p;
            if (hipEventCreate(&p.start) != hipSuccess || hipEventCreate(&p.stop) != hipSuccess) return nullptr;
            pool.push_back(p);
        }
        return &pool[prof_used[k]++];
    }
};


// HIP events around whatever is enqueued on the engine's stream during the scope's lifetime (slam_profile_*)
struct ProfScope {
    slam_engine* e;
    const EventPair* ev;
    ProfScope(slam_engine* e_, int kernel) : e(e_), ev(e_->prof_next(kernel))
    {
        if (ev) (void)hipEventRecord(ev->start, e->stream);
    }
    ~ProfScope()
    {
        if (ev) (void)hipEventRecord(ev->stop, e->stream);
    }
    ProfScope(const ProfScope&) = delete;
    ProfScope& operator=(const ProfScope&) = delete;
};

// ---- helpers shared between the translation units, by the unit that implements them
// engine.hip: what a failed HIP call leaves in slam_last_error ("what: hipGetErrorString") and returns
int slam_engine_fail_hip(slam_engine* e, hipError_t err, const char* what);
// bounded spin on a word in mapped host memory (a few seconds at most); false: it never showed `want`
inline bool slam_spin_flag(const volatile uint32_t* flag, uint32_t want)
{
    for (long spin = 0; spin < 400000000L; ++spin)
        if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) == want) return true;
    return false;
}
// engine.hip: wait until `flag` shows `seq`.  With a communicator: comm_wait_flag (polls it, bounded in time).  Without: the
// bounded spin, then a stream synchronisation and one more look; SLAM_ERR_HIP naming `what` if it still is not there.
int slam_engine_wait_flag(slam_engine* e, slam_comm* comm, const volatile uint32_t* flag, uint32_t seq, const char* what);

// engine_assoc.hip: a pending detection count (slam_detect_scan_dev) becomes e->ndet — a flag wait, no copy, no stream
// synchronisation; nothing pending: nothing happens
int slam_engine_resolve_detections(slam_engine* e);
// the conditions of slam_detect_scan_dev on its parameters (NaN fails every comparison) and what a refusal leaves in slam_last_error
inline bool slam_detect_params_ok(const slam_detect_params* p)
{
    const float big = 3.402823466e+38f;
    const float len[4] = { p->jump, p->guard, p->max_width, p->max_range };
    for (float v : len)
        if (!(v > 0.0f && v <= big)) return false;
    return p->guard >= p->jump && p->min_points >= 1 && p->min_points <= p->max_points && p->max_points <= SLAM_DETECT_MAX_POINTS &&
           (p->wrap == 0 || p->wrap == 1);
}
inline void slam_detect_params_error(slam_engine* e)
{
    snprintf(e->err, sizeof e->err, "the detector needs finite jump, guard, max_width and max_range > 0, guard >= jump, "
                                    "1 <= min_points <= max_points <= %d and wrap in {0, 1}", (int)SLAM_DETECT_MAX_POINTS);
}

// ... and of slam_detect_scan_fit_dev on a fit
inline bool slam_detect_fit_ok(const slam_detect_fit* f)
{
    const float big = 3.402823466e+38f;
    return f->radius > 0.0f && f->radius <= big && f->spread_tol >= 0.0f && f->spread_tol <= big;
}
inline void slam_detect_fit_error(slam_engine* e)
{
    snprintf(e->err, sizeof e->err, "the detector's fit needs a finite radius > 0 and a finite spread_tol >= 0");
}

// ... and of slam_detect_scan_noise_dev on a noise model
inline bool slam_detect_noise_ok(const slam_detect_noise* z)
{
    const float big = 3.402823466e+38f;
    return z->range_var > 0.0f && z->range_var <= big && z->bearing_var >= 0.0f && z->bearing_var <= big && z->lateral_var >= 0.0f &&
           z->lateral_var <= big && z->bearing_var + z->lateral_var > 0.0f;
}
inline void slam_detect_noise_error(slam_engine* e)
{
    snprintf(e->err, sizeof e->err, "the detector's noise model needs a finite range_var > 0, finite bearing_var >= 0 and lateral_var >= 0, "
                                    "and bearing_var + lateral_var > 0");
}

// The two choices a landmark update on rows has (kernels.h: launch_ekf_rows), as the engine's stages take them.
// The measurement noise: meas_var * I, or — full — the 2x2 sensor-frame covariance meas_cov[3] = {qxx, qxy, qyy}
// — or per_det — the covariances the engine's detections carry (meas_var and meas_cov are not read)
struct slam_meas_noise {
    float meas_var;
    const float* meas_cov;
    bool full;
    bool per_det = false;
};
// ... and a per-particle association table as the source of the observations (no table: the engine's observation table)
struct slam_assoc_view {
    const uint8_t* d_assoc;
    int assoc_stride;
};
// meas_cov as the 2x2 stages accept it; leaves the reason in slam_last_error otherwise
inline bool slam_aniso_cov_from(slam_engine* e, const float meas_cov[3], slam::EkfAnisoCov* q)
{
    *q = slam::ekf_aniso_cov(meas_cov);
    if (slam::ekf_aniso_cov_ok(*q)) return true;
    snprintf(e->err, sizeof e->err, "meas_cov must be finite with qxx > 0, qyy > 0 and qxx * qyy - qxy * qxy > 0 in float32");
    return false;
}
// engine_ekf.hip: slam_ekf_update_dev, _aniso_dev, _assoc_dev and _assoc_aniso_dev are this one function, their checks and status
// codes in one order: the isotropic update from the observation table alone has the sparse in-place and the grouped kernels, a
// table brings SLAM_MAX_OBS, the detections (resolved first; SLAM_ERR_NOT_READY without any) and d_assoc with it
extern "C" int slam_engine_ekf_update(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride,
                                      int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                      const slam_meas_noise& noise, const slam_assoc_view* table, float* d_loglik);
// engine_assoc.hip: slam_associate_dev and slam_associate_aniso_dev likewise
extern "C" int slam_engine_associate(slam_engine* e, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                     const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                                     const slam_meas_noise& noise, float gate, float new_gate, int create, uint8_t* d_assoc,
                                     int assoc_stride, int32_t* d_stats);

// The switches of the existence-evidence stage (kernels.h: launch_landmark_evidence), as the engine's stage takes them: which of
// the two rules spare a landmark that is due a miss.  Neither: d_th is not read
struct slam_evidence_form {
    const float* d_th = nullptr;    // [n] the headings the update used; needed under either rule
    float margin = 0.0f;            // line of sight: finite, > 0 (not read without use_sight)
    bool use_sight = false;         // line of sight against the engine's sight table (slam_sight_table_dev first)
    bool fov = false;               // a field of view: the arc lo .. hi of the diamond angle, each in [0, 4]
    float lo = 0.0f, hi = 4.0f;
    int32_t* d_spared = nullptr;    // [n] hidden; written under either rule (0 without use_sight); may be nullptr
    int32_t* d_outside = nullptr;   // [n] outside the arc; written with fov; may be nullptr
};
// engine_evidence.hip: slam_landmark_evidence[_sight | _fov][_missed]_dev are this one function, their checks and status codes in
// one order: the detections resolved first, SLAM_ERR_INVALID_ARG, SLAM_ERR_NOT_READY (no detections; line of sight without a
// table), n == 0.  Counts in the counter of its form: fov_launches with fov, else sight_launches[1] with use_sight, else
// evidence_launches[0]
__attribute__((visibility("hidden"))) int slam_engine_evidence(slam_engine* e, float* d_map, int64_t row_stride, int plane_stride,
                                                               int nlandmarks, const float* d_x, const float* d_y, const int32_t* d_anc,
                                                               int n, const uint8_t* d_assoc, int assoc_stride, const uint8_t* d_ev_in,
                                                               uint8_t* d_ev_out, int ev_stride, int hit, int miss, int cmax,
                                                               float view_range, int32_t* d_stats, int32_t* d_missed,
                                                               const slam_evidence_form& form);

// engine_reseed.hip: slam_pose_reseed_dev with its checks and status codes, and a choice of how the two counts come back.
// mapped == nullptr: by a copy behind a stream synchronisation, into counts.  Else the launch leaves them in mapped host memory
// behind a sequence number (the session waits for that word and reads them there; counts is not written) and nothing synchronises.
// *launched = false: K == 0, nothing was issued and nothing will arrive
struct slam_reseed_mapped {
    int32_t* d_hout;    // the two words as the device sees them
    uint32_t* d_hseq;
    uint32_t seq;
};
__attribute__((visibility("hidden"))) int slam_engine_pose_reseed(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks,
                                                                  const float* d_x_in, const float* d_y_in, const float* d_th_in,
                                                                  const int32_t* d_anc, float* d_x_out, float* d_y_out, float* d_th_out,
                                                                  int n, int64_t first_id, uint64_t seed, uint32_t frame, float fraction,
                                                                  uint8_t* d_flag, const slam_reseed_mapped* mapped, int32_t counts[2],
                                                                  bool* launched);

// ... and slam_pose_reseed_pairs_dev the same way (four words in mapped host memory).  *launched = false: K < 2
__attribute__((visibility("hidden"))) int slam_engine_pose_reseed_pairs(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks,
                                                                        const float* d_x_in, const float* d_y_in, const float* d_th_in,
                                                                        const int32_t* d_anc, float* d_x_out, float* d_y_out, float* d_th_out,
                                                                        int n, int64_t first_id, uint64_t seed, uint32_t frame, float fraction,
                                                                        float tol, float min_sep, uint8_t* d_flag,
                                                                        const slam_reseed_mapped* mapped, int32_t counts[4], bool* launched);

// engine_match.hip
namespace slam_detail {
// slot in range, its grid and a scan present
__attribute__((visibility("hidden"))) int check_score_inputs(slam_engine* e, int slot);
// the grid of `slot` as the scorers of `nposes` poses want it (with the byte-per-cell copy when there are many)
__attribute__((visibility("hidden"))) int many_pose_grid(slam_engine* e, int slot, int nposes, slam::ScoreGrid* out);
}  // namespace slam_detail
// engine_resample.hip:
// e->bmax_buf holds logweight_scratch_floats() floats, zeroed when it was made: in front of whichever launch leaves the block maxima
__attribute__((visibility("hidden"))) int slam_engine_bmax_ready(slam_engine* e);
// slam_logweight_dev / slam_logweight_ekf_dev (use_ekf) with, optionally, a split session's covariance classes brought up to
// date by workgroups of the same launch (launch_logweight)
extern "C" int slam_logweight_cov_dev(slam_engine* e, const float* d_score, bool use_ekf, float score_gain, int n, float* d_logw, float* d_max,
                           const slam::CovArgs* cov, int cov_bound);
// slam_quantise_scan_dev(d_max = nullptr) on one GPU with a split session's covariance classes brought up to date by workgroups
// of the same launch (launch_quantise_scan): the form for a frame whose weights the front launch made
extern "C" int slam_quantise_scan_cov_dev(slam_engine* e, const float* d_logw, int n, const slam::CovArgs* cov, int cov_bound);
// engine_ekf.hip:
// slam_motion_score_dev with a rider
extern "C" int slam_motion_score_rider_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                                           const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id,
                                           const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame, float* d_score,
                                           int32_t* d_count, const slam::FreeListRider* rider, bool* rode);
// weights (optional): the frame's log-weights may come out of the front launch as well (kernels.h: FrontWeights) — score_gain
// and d_logw as slam_logweight_cov_dev takes them; *made = true: they did, the block maxima are where slam_quantise_scan_dev
// looks for them, and the frame needs no weights' launch (its classes' update: slam_quantise_scan_cov_dev)
struct slam_front_weights {
    float score_gain;
    float* d_logw;
    bool* made;
};
// slam_motion_score_dev + slam_ekf_update_dev (out of place, through the resample indices d_anc) as ONE launch
// (launch_frame_front).  *launched = false: the shapes do not fit or fusion is off — nothing was issued, the caller makes
// the two calls.  Used by the slam_pf session for single-GPU frames on rows.
extern "C" int slam_frame_front_dev(slam_engine* e, int slot, const float* d_src_x, const float* d_src_y, const float* d_src_th,
                         const int32_t* d_anc, float* d_x, float* d_y, float* d_th, int n, int64_t first_id, const float dp[3],
                         const float sigma[3], uint64_t seed, uint32_t frame, float* d_score, int32_t* d_count,
                         const float* d_map_in, float* d_map_out, int64_t row_stride, int plane_stride, int nlandmarks,
                         float meas_var, bool* launched, const slam::SplitIO* split = nullptr, float* d_obs_save = nullptr,
                         const slam_front_weights* weights = nullptr);
// survivor rows: d_obs_save != nullptr asks slam_frame_front_dev for the launch that writes no mean row (split only) and keeps
// the observation table there ([2][plane_stride]); this is the launch that writes them later, from the same inputs — the mean
// rows of slam_ekf_split_dev bit for bit and nothing else (the stored poses; split->cov / covx: the PRIOR class rows; cls_out,
// cstamp unused).  d_survivor: only particles i with d_survivor[i] == stamp (nullptr: all).  Counts in no form counter.
extern "C" int slam_ekf_materialise_dev(slam_engine* e, const float* d_mean_in, float* d_mean_out, int64_t row_stride, int plane_stride,
                             int nlandmarks, const float* d_obs_save, const float* d_x, const float* d_y, const float* d_th,
                             const int32_t* d_anc, int n, float meas_var, const slam::SplitIO* split, const uint32_t* d_survivor,
                             uint32_t stamp, int group);
// engine_evidence.hip: a frame of a pruning session without a landmark update: the evidence follows its particles, d_out[i] = d_in[d_anc[i]] (rows of
// ev_stride bytes; bracketed as SLAM_PROF_PAGES like slam_gather_map_dev's table gathers; counted nowhere)
extern "C" int slam_evidence_gather_dev(slam_engine* e, const uint8_t* d_in, uint8_t* d_out, int ev_stride, const int32_t* d_anc, int n);
// engine_resample.hip: slam_ancestors_from_scan_dev that also marks the particles it kept (kernels.h: SurvivorOut); needs
// ancestors_from_scan_fits(n)
extern "C" int slam_ancestors_survivors_dev(slam_engine* e, int n, uint64_t seed, uint32_t frame, int32_t* d_anc,
                                            const slam::SurvivorOut* survivors);
// the out-of-place landmark update on the SPLIT layout (kernels.h: EkfArgs): d_mean_in / d_mean_out are rows of two planes
// (row_stride >= 2 * plane_stride), the covariances come per class through `split`; otherwise slam_ekf_update_dev
extern "C" int slam_ekf_split_dev(slam_engine* e, const float* d_mean_in, float* d_mean_out, int64_t row_stride, int plane_stride,
                       int nlandmarks, const float* d_x, const float* d_y, const float* d_th, const int32_t* d_anc, int n,
                       float meas_var, const slam::SplitIO* split);
// engine_match.hip:
slam::ScoreGrid slam_engine_score_grid(const slam_engine* e, int slot);
// FastMatch on grid `slot` with the beam count read from device memory (d_nbeams, at most nbeams_max) and the
// scan at d_bx/d_by; optionally mirrors the hit scratch into d_hits_persist.  Synchronises.
int slam_engine_fastmatch(slam_engine* e, int slot, const float* d_bx, const float* d_by, int nbeams_max,
                          const int32_t* d_nbeams, const float pose[3], const float res[3], float out_pose[3],
                          float* best_hits, int32_t* best_hits_size, float* best_score, float* d_hits_persist);
// ... and FastMatch(pose, res1) on slot1 followed by FastMatch2(its result, res2) on slot2 as ONE round trip
int slam_engine_fastmatch_pair(slam_engine* e, int slot1, int slot2, const float* d_bx, const float* d_by, int nbeams_max,
                               const int32_t* d_nbeams, const float pose[3], const float res1[3], const float res2[3],
                               float out_pose[3], int32_t* best_hits_size, float* d_hits_persist);

// engine_resample.hip: what slam_pose_spread_dev and slam_pf_spread return from the mean and the sums of pose_moments_kernel
// (estimate_host.h); SLAM_ERR_INVALID_ARG, with the reason in slam_last_error, when a particle lay outside the domain
__attribute__((visibility("hidden"))) int slam_engine_spread_result(slam_engine* e, const slam::PoseMean& mean, const long long m[slam::kPoseMoments],
                                                                    float pose[3], float cov[6], float* heading_r);
// engine_modes.hip: the three launches of the modes (kernels.h: launch_modes) on the engine's stream, parameters checked, the
// buffers made at the first call; the raw result (kModesWords 8-byte words) goes to device memory at *d_raw and, with d_hout, to
// mapped host memory behind *d_hseq = seq.  Then: what slam_pose_modes_dev and slam_pf_modes return from the raw words —
// SLAM_ERR_INVALID_ARG (a particle outside the domain) or SLAM_ERR_CAPACITY (too many cells) with the reason in slam_last_error
// and no output written.
__attribute__((visibility("hidden"))) int slam_engine_modes_launch(slam_engine* e, const float* d_x, const float* d_y, const float* d_theta,
                                                                   const int32_t* d_idx, const float* d_carry, int n, float ref_theta, float cell,
                                                                   int hbins, int max_modes, long long* d_hout, uint32_t* d_hseq, uint32_t seq,
                                                                   const long long** d_raw);
__attribute__((visibility("hidden"))) int slam_engine_modes_result(slam_engine* e, const long long* raw, float ref_theta, float cell,
                                                                   slam_pf_mode* modes, int* n_modes, int* cells, int64_t* wtotal);
// engine_resample.hip: slam_migrate_pack_dev for a session with paged maps (d_pt: page tables of nb entries, d_map: the page pool)
extern "C" int slam_migrate_pack_paged(slam_engine* e, int n_local, int rank, int world, const int32_t* plan, const float* d_pose,
                            int64_t pose_ld, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                            float* d_out, const int32_t* d_pt, int nb, const float* d_split_cov = nullptr,
                            const int32_t* d_split_cls = nullptr,   // split layout: d_map = the means (row_stride >= 2 planes)
                            const slam::PageGeom* geom = nullptr);   // split pages (d_pt and d_split_cls): d_map = the pool of mean pages

#define SLAM_HIP_TRY(e, call)                                                     \
    do {                                                                          \
        hipError_t err__ = (call);                                                \
        if (err__ != hipSuccess) return slam_engine_fail_hip((e), err__, #call); \
    } while (0)

// first line of every entry point that takes the engine
#define SLAM_ENTER(e)                                  \
    do {                                               \
        if (!(e)) return SLAM_ERR_INVALID_ARG;         \
        SLAM_HIP_TRY((e), hipSetDevice((e)->device)); \
    } while (0)
