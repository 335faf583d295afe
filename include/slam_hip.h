/*
 * slam_hip.h — C ABI of the MI355X (gfx950) scan-matching / particle-filter engine.
 *
 * This is the drop-in boundary for the hot path of circuitpotato/Hardware-Acceleration-of-LIDAR-SLAM:
 * the functions below replace, one stage per call, what Subsystem_1/main_accelerated.c does in
 *   euclidean_distance_transform / euclidean_distance_transform2   (main_accelerated.c:215-283)
 *   FastMatch / FastMatch2                                        (main_accelerated.c:396-824)
 * and add the particle-filter stages the north star asks for around them (motion sample,
 * per-particle x per-landmark 2x2 EKF, weight normalisation, systematic resample), for which the
 * reference has no code.  INTEGRATION.md shows the edits a maintainer of the
 * reference makes to call these from main_accelerated.c.
 *
 * Conventions
 *  - plain C, no C++/torch types; every function returns a slam_status (0 = OK, < 0 = error) and
 *    never aborts or exits (the reference's functions are all `void` and print-and-continue,
 *    main.c:15-20; we return codes instead).
 *  - `slam_engine` is an opaque handle created once and passed to every call — the same shape as the
 *    `accel` handle the reference's FPGA variant threads through OccupationalGrid/EDT
 *    (Submodule_2/Hadrware_acclereated.cpp:236,260,284,842-845).  One engine per host thread / GPU;
 *    calls on one engine are serialised on one HIP stream.
 *  - `*_host` entry points take caller-owned HOST buffers (as the reference's functions do), copy,
 *    launch, copy back and synchronise.  `*_dev` entry points take DEVICE pointers, are asynchronous
 *    on the engine's stream and keep everything resident in HBM; they are what a frame loop with
 *    many particles uses.  The boundary is crossed once per frame stage, never per element (the
 *    reference's FPGA path crossed it once per distance, Hadrware_acclereated.cpp:223-233).
 *  - there is NO CPU fallback: if no gfx950 device is usable the calls fail with SLAM_ERR_NO_DEVICE.
 *  - float arithmetic of the reference-pinned stages (EDT, score) is bit-exact with the reference:
 *    same operation order, no FMA contraction.
 */
#ifndef SLAM_HIP_H
#define SLAM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SLAM_ABI_VERSION 5

typedef enum {
    SLAM_OK = 0,
    SLAM_ERR_NO_DEVICE = -1,   /* no usable gfx950 GPU / HIP runtime error at init */
    SLAM_ERR_INVALID_ARG = -2, /* null pointer, negative size, slot out of range, ... */
    SLAM_ERR_HIP = -3,         /* a HIP runtime call failed; slam_last_error() has the text */
    SLAM_ERR_NOT_READY = -4,   /* stage called before its inputs were provided (e.g. no grid in slot) */
    SLAM_ERR_CAPACITY = -5,    /* request exceeds a fixed capacity (beams, lattice size, ...) */
    SLAM_ERR_COMM = -6         /* an exchange between ranks failed (RCCL error, or a rank of an in-process group
                                  did not arrive); slam_last_error() has the text */
} slam_status;

typedef struct slam_engine slam_engine;

/* Bookkeeping of one occupancy/EDT grid: the fields the reference keeps beside each grid in
 * `MyGrid` (main.c:200-213): grid_size{rows,cols}, pixel_size, top_left_corner; `ld` is the leading
 * dimension of the row-major storage (fixed 200 / 400 in the reference). */
typedef struct {
    int32_t rows, cols, ld;
    float pixel;
    float min_x, min_y;
} slam_grid_meta;

/* ------------------------------------------------------------------ engine lifetime */

int slam_abi_version(void);
const char *slam_status_string(int status);
/* text of the most recent HIP error seen by this engine (empty string if none); e == NULL: why the calling thread's last
 * slam_engine_create failed */
const char *slam_last_error(const slam_engine *e);

/* device: HIP device ordinal.  Fails with SLAM_ERR_NO_DEVICE when there is none.
 * A host that times its first frames should know: the engine makes ONE allocation of pinned host memory here (every mapped
 * result buffer and the upload staging ring are carved out of it), and the driver answers such an allocation some 10-50 ms
 * later by holding the process's queues for 65-80 ms (profiles/r03_stall_trigger.txt).  Results are
 * unaffected; 50 ms between slam_engine_create and the first timed frame keep the hold out of the timing (bench.py sleeps
 * 250 ms).  Creating and destroying sessions on a live engine allocates no pinned memory. */
int slam_engine_create(int device, slam_engine **out);
int slam_engine_destroy(slam_engine *e);
/* Run the engine on a caller-provided hipStream_t (e.g. the framework's current stream) instead of
 * its own.  NULL means what it means to HIP: the default (null) stream.  SLAM_OWN_STREAM restores the
 * engine's own non-blocking stream (the initial state). */
#define SLAM_OWN_STREAM ((void *)(intptr_t)-1)
int slam_engine_set_stream(slam_engine *e, void *hip_stream);
int slam_engine_sync(slam_engine *e);

/* Per-kernel timing with HIP events recorded on the engine's stream around the named kernel's
 * launches only (not around host work or neighbouring kernels).  Off by default.  `mask` selects the
 * kernels: bit k = slam_prof_kernel k (an event pair costs a few microseconds of stream time per launch,
 * so time only what you need); 0 switches timing off.  slam_profile_read
 * synchronises the stream, returns the summed duration and the launch count since the last reset
 * and resets the counters.  (The reference's only timer is clock() around the whole run,
 * main.c:826-827, 971-973.) */
typedef enum {
    SLAM_PROF_SCORE = 0,        /* score_poses_kernel (with or without the motion sample), lattice kernels */
    SLAM_PROF_EDT = 1,          /* edt kernels */
    SLAM_PROF_EKF = 2,          /* the landmark update of a frame, whichever kernel runs it (rows, grouped, list, pages) */
    SLAM_PROF_WEIGHTS = 3,      /* log-weights + block maxima (+ the maximum's finalize launch on several GPUs); a split session's
                                   covariance classes are brought up to date by workgroups of the same launch.  A survivor-rows frame
                                   whose fused front launch made the weights itself has no launch in this bracket */
    SLAM_PROF_SCAN = 4,         /* quantise + prefix sum (+ ESS sums); + the covariance classes' update on a frame without a weights' launch */
    SLAM_PROF_ANCESTORS = 5,    /* offspring offsets / ancestor search (single GPU: one launch) */
    SLAM_PROF_PLAN = 6,         /* several GPUs: global ancestor search, flag scans, exchange plan, local gather index */
    SLAM_PROF_PACK = 7,         /* several GPUs: migrating rows into the send buffer */
    SLAM_PROF_UNPACK = 8,       /* several GPUs: received rows into the staging tail */
    SLAM_PROF_COLLECTIVES = 9,  /* every exchange between ranks (all-reduce, all-gathers, send/recv), as the stream sees them */
    SLAM_PROF_PAGES = 10,       /* map bookkeeping: data association (slam_associate_dev), existence evidence (slam_landmark_evidence_dev), paged maps' touched-page list, table gathers, the free list where it is a launch of
                                   its own (one GPU: it travels in the scorer's launch); split maps' gathers on frames without observations */
    SLAM_PROF_EKF_TAIL = 11,    /* several GPUs, split maps: the part of the landmark update that waits for the exchange (the
                                   groups with an ancestor in the staging tail); the rest went out with the score (SLAM_PROF_EKF) */
    SLAM_PROF_MATERIALISE = 12, /* survivor rows (slam_survivor_rows_set): the launch behind the resample that writes the mean rows of
                                   the particles it kept, and the launch that writes all of them when something asks (settle) */
    SLAM_PROF_COUNT = 13
} slam_prof_kernel;
int slam_profile_enable(slam_engine *e, int mask);
int slam_profile_read(slam_engine *e, int kernel, double *total_ms, int64_t *launches);
/* What an EMPTY start/stop bracket measures on this stream (mean of 64 back-to-back pairs, ms): the part of a
 * bracketed duration that is event bookkeeping rather than kernel time.  Synchronises. */
int slam_profile_bracket_overhead(slam_engine *e, double *overhead_ms);
/* What a PURE COPY with the landmark update's access shape reaches on this GPU: `rows` rows of five planes of
 * `plane_stride` floats (a multiple of 128) are copied from d_src to d_dst `reps` times (one wavefront per row, 256-byte
 * wave accesses, all loads of two batches before their stores, XCD-contiguous workgroup numbering, streaming stores —
 * the addressing of the update without its arithmetic); *ms_per_copy is the average duration from HIP events.  Any
 * kernel that reads 20 B and writes 20 B per (particle, landmark) is bounded by it: measurement support, not a stage. */
/* Self-check of the landmark update's reciprocal (csrc/ekf_math.h): the update computes 1 / det without the scaling and
 * fix-up steps of a general IEEE division whenever det's exponent lies in [-60, 60]; this walks every float of that range
 * on the device (2 x 121 x 2^23 values) and compares with the compiler's correctly rounded division.  *mismatches must
 * come back 0. */
int slam_selftest_reciprocal(slam_engine *e, int64_t *mismatches, int64_t *checked);
int slam_profile_copy_ceiling(slam_engine *e, const float *d_src, float *d_dst, int64_t rows, int plane_stride, int reps,
                              double *ms_per_copy);

/* ------------------------------------------------------------------ EDT */

/* Capped exact Euclidean distance transform of occ[0..rows)[0..cols) (row-major, leading dimension
 * ld, non-zero = occupied): out = 0 on occupied cells, else min(cap, sqrtf(min d^2)) in cells; cells
 * outside rows x cols are not written.  Replaces euclidean_distance_transform{,2}
 * (main.c:223-269, main_accelerated.c:215-283). */
int slam_edt_dev(slam_engine *e, const int32_t *d_occ, int ld, int rows, int cols, float cap, float *d_out);
int slam_edt_host(slam_engine *e, const int32_t *occ, int ld, int rows, int cols, float cap, float *out);

/* ------------------------------------------------------------------ engine-resident grids + scan
 * (what the reference keeps in the globals `occ_grid` and `scan`) */

enum { SLAM_MAX_GRID_SLOTS = 4, SLAM_MAX_BEAMS = 4096 };

/* Upload an occupancy grid, build its EDT on the device and keep it as grid `slot` (0 = the coarse
 * grid FastMatch reads, 1 = the fine grid FastMatch2 reads).  When edt_out != NULL the EDT is also
 * copied back in the same [.. ][ld] layout (only the rows x cols rectangle is written).
 * = the tail of OccupationalGrid (main.c:355-362). */
int slam_grid_upload_host(slam_engine *e, int slot, const int32_t *occ, const slam_grid_meta *meta, float cap,
                          float *edt_out);
/* Replace pixel / min_x / min_y of a grid already in `slot` (rows, cols, ld must be unchanged).  The
 * reference runs its EDTs before it records pixel_size and top_left_corner (main.c:355-362); an
 * adapter with the reference's EDT signature therefore learns them one step later. */
int slam_grid_set_meta(slam_engine *e, int slot, const slam_grid_meta *meta);
/* Adopt an EDT that is already on the device (not copied; caller keeps it alive).
 * The scorers of many poses (slam_score_poses_*, slam_motion_score_dev, slam_pf_step with >= 3 072 poses) gather from a packed
 * copy of the grid — one byte per cell, made on their first call after the grid changed (the capped EDT holds only 0,
 * sqrtf of small integers and the cap: main.c:223-269; a grid with other values keeps the float path) — so call
 * slam_grid_set_dev again after rewriting the cells of an adopted grid (slam_edt_dev into the adopted buffer is noticed
 * by itself).  Results are bit-identical either way. */
int slam_grid_set_dev(slam_engine *e, int slot, const float *d_edt, const slam_grid_meta *meta);
/* Where grid `slot` stands with its packed copy: *state = 0: no verdict since the grid last changed (upload, adoption,
 * slam_edt_dev into the adopted buffer) — no scorer of >= 3 072 poses has read it since, or the grid has fewer than 8 rows or
 * 16 columns; 1: the packed copy is in use; 2: the grid does not pack (a cell that is neither sqrtf of an integer 0 .. 254 nor
 * the grid's largest value) and the scorers keep the float grid.  slam_grid_set_meta leaves the state as it is.  A capped EDT
 * packs at every cap up to 16.0 (its distances below the cap are sqrtf of at most 250); with a larger cap it packs as long as
 * its cells of 16.0 and more all hold one value.  Reads host bookkeeping only: no launch, no wait.  SLAM_ERR_NOT_READY:
 * nothing in the slot. */
int slam_grid_packed_state(slam_engine *e, int slot, int *state);
/* Sensor-frame cartesian beams of the current scan = scan.x / scan.y (main.c:60-69). */
int slam_scan_upload_host(slam_engine *e, const float *bx, const float *by, int nbeams);
int slam_scan_set_dev(slam_engine *e, const float *d_bx, const float *d_by, int nbeams);

/* ------------------------------------------------------------------ scan-match score (row A7) */

/* Score every pose against grid `slot` with the current scan:
 *   score[i] = in-order float sum of EDT[cell(pose_i (+) beam_b)] over in-bounds beams,
 *   count[i] = number of in-bounds beams                       (main.c:459-518, Appendix A.5).
 * Heading trig: the `_cs` form takes cos/sin per pose computed by the caller (the reference computes
 * them with libm on the host, main.c:433-435; this form is bit-exact with the reference for any
 * pose); the theta form computes them on the device with the engine's specified polynomial
 * (DESIGN.md "device trig"), bit-exact with the oracle's restatement of the same polynomial. */
int slam_score_poses_cs_dev(slam_engine *e, int slot, const float *d_x, const float *d_y, const float *d_ct,
                            const float *d_st, int nposes, float *d_score, int32_t *d_count);
int slam_score_poses_dev(slam_engine *e, int slot, const float *d_x, const float *d_y, const float *d_theta,
                         int nposes, float *d_score, int32_t *d_count);
int slam_score_poses_cs_host(slam_engine *e, int slot, const float *x, const float *y, const float *ct,
                             const float *st, int nposes, float *score, int32_t *count);
int slam_score_poses_host(slam_engine *e, int slot, const float *x, const float *y, const float *theta, int nposes,
                          float *score, int32_t *count);
/* In-bounds EDT values of ONE pose in beam order (what the reference leaves in
 * FastMatchParameters.bestHits, main.c:515); hits must hold nbeams floats. */
int slam_pose_hits_host(slam_engine *e, int slot, float x, float y, float ct, float st, float *hits, int32_t *count);

/* Drop-in for FastMatch (slot 0) / FastMatch2 (slot 1), main.c:381-596 / 598-809, quirks included:
 * 27-pose lattice laid out once around `pose` with step res[0] in x AND y and res[2] in theta
 * (res[1] is never read), strict '<' arg-min in theta-major, x, y-minor order; *best_hits_size =
 * in-bounds count of the BEST candidate while best_hits[] is left as the reference leaves its shared
 * scratch: every candidate overwrote the prefix [0, its count), last writer wins, entries beyond the
 * longest candidate keep the caller's previous content.  best_hits must hold
 * nbeams floats and should persist between calls like FastMatchParameters.bestHits; best_score may
 * be NULL. */
int slam_fastmatch_host(slam_engine *e, int slot, const float pose[3], const float res[3], float out_pose[3],
                        float *best_hits, int32_t *best_hits_size, float *best_score);

/* ------------------------------------------------------------------ particle-filter stages
 * (rows A9-A12: no counterpart in the reference; specified in DESIGN.md and oracle/slam_oracle_pf.c).
 * Particles are SoA float arrays x[], y[], theta[]; `first_id` is the global index of element 0 of
 * this shard (0 on a single GPU) so that results do not depend on how particles are sharded. */

/* A9: x,y,theta[i] = src(x,y,theta)[anc ? anc[i] : i] + dp + eps_i, eps ~ N(0, diag(sigma^2)) from
 * Philox4x32-10 keyed (seed, frame) and countered by the global particle id.  With sigma = 0 this
 * is the reference's constant-velocity predict (main.c:875-898) applied to every particle.
 * d_anc (may be NULL) are LOCAL indices into the source arrays (resample gather fused in). */
int slam_motion_sample_dev(slam_engine *e, const float *d_src_x, const float *d_src_y, const float *d_src_th,
                           const int32_t *d_anc, float *d_x, float *d_y, float *d_th, int n, int64_t first_id,
                           const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame);

/* A9 + A7 in one launch: the motion sample above followed by the scan-match score of the new poses
 * (same results as slam_motion_sample_dev then slam_score_poses_dev; source and destination arrays
 * must differ). */
int slam_motion_score_dev(slam_engine *e, int slot, const float *d_src_x, const float *d_src_y,
                          const float *d_src_th, const int32_t *d_anc, float *d_x, float *d_y, float *d_th, int n,
                          int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame,
                          float *d_score, int32_t *d_count);

/* Scan-match refinement of every pose ("Refinement"): `sweeps` (1..16) sweeps of the reference's
 * 3 x 3 x 3 lattice (FastMatch, main.c:424-563) around EACH pose, in one launch.  One sweep: candidates theta -/+ step_theta,
 * x -/+ step_xy, y -/+ step_xy (one binary32 subtract or add each), every candidate scored exactly as slam_score_poses_dev
 * scores that pose (headings through the particle path's deterministic sincos, not libm), the centre as the incumbent:
 * the candidates are visited heading-major, x, y-minor like the reference's, and one replaces the incumbent only with a
 * strictly lower score — unlike FastMatch, which starts from +inf and walks to candidate 0 when all 27 tie, a pose in free
 * space or off the grid stays where it is.  The pose becomes the winner and the next sweep is laid around it.  Like the
 * weights, the comparison is on the raw sum: a candidate with fewer in-bounds beams can win (the reference's behaviour,
 * SURVEY Q-list).  d_x / d_y / d_th are read and overwritten with the final pose, d_score / d_count receive its score and
 * in-bounds count.  Steps must be finite and >= 0; n == 0 launches nothing.  Bracketed as SLAM_PROF_SCORE. */
int slam_refine_poses_dev(slam_engine *e, int slot, float *d_x, float *d_y, float *d_th, int n, float step_xy,
                          float step_theta, int sweeps, float *d_score, int32_t *d_count);
/* slam_motion_sample_dev followed by the above, one launch (the unrefined sample is never stored); source and destination
 * arrays must differ */
int slam_motion_refine_dev(slam_engine *e, int slot, const float *d_src_x, const float *d_src_y, const float *d_src_th,
                           const int32_t *d_anc, float *d_x, float *d_y, float *d_th, int n, int64_t first_id,
                           const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame, float step_xy,
                           float step_theta, int sweeps, float *d_score, int32_t *d_count);

/* A10: per-particle x per-landmark 2x2 EKF correction (FastSLAM 1.0, known correspondences,
 * cartesian sensor-frame observations z = H (m - t), H = [[ct,-st],[st,ct]], noise R = meas_var * I).  H being a rotation
 * and R isotropic, the update is carried out in the world frame: w = t + H^T z, S = P + R, W = P S^-1, mu' = mu + W (w - mu),
 * P' = (I - W) P, log-likelihood term -1/2 (w - mu)^T S^-1 (w - mu) - 1/2 log det S - log 2 pi — the sensor-frame Kalman
 * update in other words, in the fixed operation order of csrc/ekf_math.h == oracle/slam_oracle_pf.c.
 * The observations of the current frame are sensor data like the scan: hand them over once per frame,
 * either as a list from the host (slam_obs_upload_host: landmark ids unique and < nlandmarks, no NaN
 * measurements, nlandmarks <= SLAM_MAX_OBS) or as a table that is already on the device
 * (slam_obs_set_dev).  Inside the engine they are a table indexed by landmark either way.
 * The map is ONE ROW PER PARTICLE: value (plane p, landmark l) of particle i lives at
 * d_map[i * row_stride + p * plane_stride + l], planes mu_x, mu_y, P_xx, P_xy, P_yy, strides in floats
 * (plane_stride >= nlandmarks, row_stride >= 5 * plane_stride; plane_stride a multiple of 32 keeps every
 * row 128-byte aligned and is what the engine's own session uses).  For every observed landmark: read
 * the 5 values of row src(i), update, write them to row i of the output map.  With d_anc != NULL the
 * resample gather is fused in (src(i) = anc[i], a local index; requires d_map_in != d_map_out);
 * landmarks without an observation are copied through when the update is out of place.  P_xx < 0 marks
 * a landmark not seen yet: it is initialised from the observation and contributes no likelihood.
 * The padding columns [nlandmarks, plane_stride) of an output row are unspecified after an out-of-place
 * update (whole 128-landmark batches that fit into the row are processed without predication, padding
 * included, so a plane_stride that is a multiple of 128 is the fastest).
 * loglik[i] (overwritten) is the sum of the observation log-likelihoods in a fixed order: landmark l adds
 * its term to accumulator l mod 128 in order of l (nothing for a landmark without an observation),
 * accumulators j and j+64 are added, and the 64 sums are reduced by a 6-level xor butterfly
 * (t[j] += t[j ^ s], s = 1..32).  The order of the observation list does not matter. */
enum { SLAM_MAX_OBS = 8192 };
int slam_obs_upload_host(slam_engine *e, const int32_t *landmark_id, const float *zx, const float *zy, int nobs,
                         int nlandmarks);
/* Observations already on the device, as the table the engine works on: entry l of the two arrays is the
 * observation of landmark l, NaN in d_zx_by_landmark[l] = landmark l was not observed this frame.  Nothing is
 * copied: the arrays must stay valid until the EKF call that uses them has run.  Their contents may be rewritten
 * between launches without another slam_obs_set_dev: every launch reads them afresh (stream-ordered). */
int slam_obs_set_dev(slam_engine *e, const float *d_zx_by_landmark, const float *d_zy_by_landmark, int nlandmarks);
/* d_loglik may be NULL: the log-likelihoods always stay inside the engine as well, where
 * slam_logweight_ekf_dev picks them up. */
int slam_ekf_update_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t row_stride, int plane_stride,
                        int nlandmarks, const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc,
                        int n, float meas_var, float *d_loglik);

/* The out-of-place update has two kernels that give the SAME bits: one wavefront per particle (neighbouring particles
 * share their ancestor's row through L2), and one wavefront per 2 or 4 neighbouring particles (the shared row stays in
 * registers).  form = -1 (the initial state): the engine chooses — grouped whenever the update gathers through resample
 * indices, 4 particles per wavefront when its last resample stage reported few distinct ancestors, else 2; 0 forces the
 * first kernel, 1 / 2 the second with 4 / 2 particles per wavefront (tests, measurements). */
int slam_ekf_form_set(slam_engine *e, int form);
/* out-of-place EKF launches of this engine so far: counts[0] one wavefront per particle, counts[1] the grouped kernel
 * (by itself or inside the fused front launch below) */
int slam_ekf_form_counts(slam_engine *e, int64_t counts[2]);
/* GENERAL MEASUREMENT COVARIANCE.  slam_ekf_update_dev is the update for R = meas_var * I.  This is the same stage for a full
 * 2x2 covariance Q = [[qxx, qxy], [qxy, qyy]] of the observation IN THE SENSOR FRAME (meas_cov = {qxx, qxy, qyy}): a lidar's
 * range and bearing noise differ by orders of magnitude.  In the world frame the noise is R_w = H^T Q H, H^T = [[c, s],
 * [-s, c]] with (s, c) the deterministic sine / cosine of the particle's heading, so the posterior covariance depends on
 * the particle: the stage exists on the row layout only.  With S = P + R_w, d = w - mu and w the observed point in the world
 * frame:  mu' = w - R_w S^-1 d,  P' = (det P * R_w + det Q * P) / det S,  log-likelihood -1/2 d^T S^-1 d - 1/2 log det S
 * - log 2 pi; a first sighting stores w and P = R_w.  Operation order: tests/_aniso_spec.py, csrc/ekf_aniso_math.h.
 * Arguments, argument checks, observation table, forms (d_anc with d_map_in != d_map_out: out of place, unobserved landmarks
 * copied; d_map_in == d_map_out and d_anc == NULL: in place, only observed landmarks touched), the log-likelihood's
 * summation order and where it stays (slam_logweight_ekf_dev), padding columns and the SLAM_PROF_EKF bracket are those of
 * slam_ekf_update_dev.  SLAM_ERR_INVALID_ARG unless every value of meas_cov is finite, qxx > 0, qyy > 0 and
 * qxx * qyy - qxy * qxy, worked out in float32, is > 0.  One kernel (a wavefront per particle); its launches are counted
 * by slam_ekf_aniso_count and in neither slam_ekf_form_counts nor slam_ekf_inplace_form_counts. */
int slam_ekf_update_aniso_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc,
                              int n, const float meas_cov[3] /* qxx, qxy, qyy */, float *d_loglik);
int slam_ekf_aniso_count(slam_engine *e, int64_t *launches);
/* DATA ASSOCIATION.  slam_ekf_update_dev needs to be told which landmark every observation belongs to; a feature detector
 * delivers points in the sensor frame with no identity attached.  These stages let every particle decide for itself (rows
 * only: a table per particle means that the landmarks a frame observes differ between particles).  The DETECTIONS of a frame
 * are handed over once, like the observation table: from the host (finite values; copied) or as two device arrays (adopted,
 * read afresh by every launch), 0 <= ndet <= SLAM_MAX_DETECTIONS.
 * slam_associate_dev, for particle i with row src = d_anc[i] (NULL: i) of d_map, pose (x, y, th)_i, q = meas_var:
 *   a. w_k = the observed point of detection k in the world frame (the update's own: t + H^T z);
 *   b. a landmark l < nlandmarks is SEEN unless P_xx < 0 (the update's first-sighting test); for a seen one and every k,
 *      m(l, k) = d^T (P + q I)^-1 d with d = w_k - mu: the very Mahalanobis term of the update's likelihood, same operations;
 *   c. the landmark chooses k*(l) = argmin_k m(l, k) (lowest k on ties) and is a candidate iff 0 <= m(l, k*) <= gate (float
 *      comparisons: NaN never passes);
 *   d. the detection chooses: of the candidates with k*(l) = k the one with the smallest m (lowest l on ties) gets
 *      assoc[l] = k, the others get nothing this frame — no landmark holds two detections, no detection serves two landmarks;
 *   e. create != 0: a detection that is unmatched and has no seen landmark with m(l, k) <= new_gate is NEW; the new
 *      detections in ascending k take the unseen landmarks (P_xx < 0) in ascending l, and once those run out the rest is
 *      dropped.  The update's first-sighting path then initialises such a landmark (mean = w_k, P = q I, no likelihood term).
 * d_assoc is uint8 [n][assoc_stride]: entry l = k or SLAM_ASSOC_NONE, the columns [nlandmarks, assoc_stride) are
 * SLAM_ASSOC_NONE.  d_stats (may be NULL) is int32 [n][3] = matched, created, dropped (every detection that is neither).
 * The rows are not written.  Operation order: tests/_assoc_spec.py.
 * slam_ekf_update_assoc_dev is slam_ekf_update_dev with particle i's own observation list {(l, z[d_assoc[i][l]]) :
 * d_assoc[i][l] != SLAM_ASSOC_NONE} (an entry that names no detection counts as SLAM_ASSOC_NONE): forms (out of place through
 * d_anc, unassociated landmarks copied; in place with d_anc == NULL, only associated landmarks touched), first sightings,
 * padding columns, the log-likelihood's summation order and where it stays (slam_logweight_ekf_dev) are unchanged.
 * SLAM_ERR_INVALID_ARG, nothing launched: gate not finite or <= 0, new_gate < gate or NaN, meas_var <= 0, nlandmarks >
 * SLAM_MAX_OBS, assoc_stride < nlandmarks, create not 0 or 1, a gather index with d_map_in == d_map_out.  SLAM_ERR_NOT_READY:
 * no detections were handed over.  ndet == 0 is legal: the table is all SLAM_ASSOC_NONE and the update copies.
 * Timing: the update is bracketed as SLAM_PROF_EKF, the association as SLAM_PROF_PAGES (map bookkeeping).  The launches are
 * counted by slam_assoc_counts (counts[0] associate, counts[1] update) and in none of the form counters. */
enum { SLAM_MAX_DETECTIONS = 64, SLAM_ASSOC_NONE = 255 };
int slam_detections_upload_host(slam_engine *e, const float *zx, const float *zy, int ndet);
int slam_detections_set_dev(slam_engine *e, const float *d_zx, const float *d_zy, int ndet);
int slam_associate_dev(slam_engine *e, const float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                       const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                       float meas_var, float gate, float new_gate, int create,
                       uint8_t *d_assoc, int assoc_stride, int32_t *d_stats /* may be NULL */);
int slam_ekf_update_assoc_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t row_stride, int plane_stride,
                              int nlandmarks, const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc,
                              int n, float meas_var, const uint8_t *d_assoc, int assoc_stride, float *d_loglik);
int slam_assoc_counts(slam_engine *e, int64_t counts[2]);
/* DATA ASSOCIATION UNDER A 2x2 MEASUREMENT COVARIANCE.  The two stages above gate and update with meas_var * I; these are the
 * same two stages for the Q of slam_ekf_update_aniso_dev (meas_cov = {qxx, qxy, qyy} in the sensor frame, the same conditions):
 * every particle gates, matches, creates and updates with S = P + R_w(theta_i), R_w = H^T Q H of its own heading.
 * slam_associate_aniso_dev is slam_associate_dev with step b reading m(l, k) = d^T (P + R_w)^-1 d — the very Mahalanobis term of
 * slam_ekf_update_aniso_dev's likelihood, same operations, the same reciprocal; steps a and c .. e, the table, the stats and the
 * rows (not written) are unchanged.  slam_ekf_update_assoc_aniso_dev is slam_ekf_update_aniso_dev with particle i's own
 * observation list read through its table row, as slam_ekf_update_assoc_dev reads it: a landmark the association created starts
 * with mean = w_k and P = R_w(theta_i) of the particle that created it, no likelihood term.  Operation order:
 * tests/_assoc_aniso_spec.py.
 * Errors: the union of the parents'.  SLAM_ERR_INVALID_ARG, nothing launched: a meas_cov that slam_ekf_update_aniso_dev refuses
 * (slam_last_error: "meas_cov must be finite ..."), and whatever slam_associate_dev / slam_ekf_update_assoc_dev refuse.
 * SLAM_ERR_NOT_READY: no detections were handed over; a detector's pending count is picked up first, as there.
 * Timing: the association is bracketed as SLAM_PROF_PAGES, the update as SLAM_PROF_EKF.  The launches are counted by
 * slam_assoc_aniso_counts (counts[0] associate, counts[1] update) and by no other counter — not slam_assoc_counts, not
 * slam_ekf_aniso_count, none of the form counters. */
int slam_associate_aniso_dev(slam_engine *e, const float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                             const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                             const float meas_cov[3] /* qxx, qxy, qyy */, float gate, float new_gate, int create,
                             uint8_t *d_assoc, int assoc_stride, int32_t *d_stats /* may be NULL */);
int slam_ekf_update_assoc_aniso_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t row_stride, int plane_stride,
                                    int nlandmarks, const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc,
                                    int n, const float meas_cov[3], const uint8_t *d_assoc, int assoc_stride, float *d_loglik);
int slam_assoc_aniso_counts(slam_engine *e, int64_t counts[2]);
/* DATA ASSOCIATION UNDER A MEASUREMENT COVARIANCE PER DETECTION.  A lidar's noise is small along the beam and larger across it,
 * and the cross-beam part grows with range: in the sensor's x/y frame that is a different 2x2 matrix for every detection.  Each
 * of the engine's current detections may therefore carry Q_k = {qxx[k], qxy[k], qyy[k]} in the sensor frame.
 * slam_detections_cov_upload_host / slam_detections_cov_set_dev attach covariances to the detections handed over last (a
 * detector's pending count is picked up first): ndet must equal the engine's ndet (else SLAM_ERR_INVALID_ARG; no detections at
 * all: SLAM_ERR_NOT_READY).  The host form checks every Q_k by the rule of slam_ekf_update_aniso_dev's meas_cov (finite, qxx > 0,
 * qyy > 0, qxx * qyy - qxy * qxy > 0 in float32; a bad one: SLAM_ERR_INVALID_ARG, nothing changes); the device form adopts the
 * three arrays as slam_detections_set_dev adopts its two, and whoever filled them answers for that rule.  det Q_k is never an
 * input: whoever uses Q_k computes t0 = qxx * qyy, t1 = qxy * qxy, detq = t0 - t1 in float32.  Whatever installs new detections
 * (slam_detections_upload_host / _set_dev, slam_detect_scan_dev / _fit_dev) installs them WITHOUT covariances: those calls do
 * exactly what they did and the covariance state is dropped.  slam_detections_get_cov_host reads the covariances back (ndet
 * values each; synchronises; SLAM_ERR_NOT_READY without any).
 * slam_associate_detcov_dev / slam_ekf_update_assoc_detcov_dev are slam_associate_aniso_dev / slam_ekf_update_assoc_aniso_dev
 * without the meas_cov argument and with Q_k in the place of Q, and nothing else changes: particle i forms R_w(i, k) =
 * H^T Q_k H of its own heading, step b reads m(l, k) = d^T (P + R_w(i, k))^-1 d per (landmark, detection) pair — still the very
 * Mahalanobis term of the likelihood the update computes for that pair, through the same reciprocal — the update of landmark l
 * runs with R_w(i, d_assoc[i][l]) and det Q of that detection, and a landmark a detection creates starts with P = R_w(i, k) of
 * that detection.  Operation order: tests/_assoc_detcov_spec.py.
 * Errors: those of the parents; SLAM_ERR_NOT_READY also when the detections carry no covariances.  Timing: the association is
 * bracketed as SLAM_PROF_PAGES, the update as SLAM_PROF_EKF.  The launches are counted by slam_assoc_detcov_counts (counts[0]
 * associate, counts[1] update) and by no other counter. */
int slam_detections_cov_upload_host(slam_engine *e, const float *qxx, const float *qxy, const float *qyy, int ndet);
int slam_detections_cov_set_dev(slam_engine *e, const float *d_qxx, const float *d_qxy, const float *d_qyy, int ndet);
int slam_detections_get_cov_host(slam_engine *e, float *qxx, float *qxy, float *qyy, int32_t *ndet);
int slam_associate_detcov_dev(slam_engine *e, const float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                              const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                              float gate, float new_gate, int create,
                              uint8_t *d_assoc, int assoc_stride, int32_t *d_stats /* may be NULL */);
int slam_ekf_update_assoc_detcov_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t row_stride, int plane_stride,
                                     int nlandmarks, const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc,
                                     int n, const uint8_t *d_assoc, int assoc_stride, float *d_loglik);
int slam_assoc_detcov_counts(slam_engine *e, int64_t counts[2]);
/* EXISTENCE EVIDENCE.  A detector produces false detections; with association alone each one that lies far from every landmark
 * takes an unseen slot and keeps it for good.  Every particle therefore keeps one EVIDENCE byte c in [0, cmax] per landmark slot
 * beside its row (uint8 [rows][ev_stride]); the counter goes up when the landmark is matched, down when it should have been
 * seen and was not, and a landmark that runs out is removed.  slam_landmark_evidence_dev runs AFTER the update of the frame
 * (slam_ekf_update_assoc_dev), for particle i and landmark l < nlandmarks, with
 *   (mu_x, mu_y, P_xx) of row i of d_map as the update left it, (px, py) = (d_x[i], d_y[i]) the pose the update used,
 *   c = d_ev_in[src][l] as an integer with src = d_anc[i] (NULL: i), a = d_assoc[i][l], K = the ndet of the engine's current
 *   detections, hit / miss / cmax integers in 1 .. 255 and range2 = view_range * view_range rounded once to float32:
 *   seen     = !(P_xx < 0)          (the update's own test: -0.0 counts as seen)
 *   hit_now  = a < K                (a byte that names no detection of this frame, K <= a <= 255, is no hit — as in the update)
 *   visible  = r2 <= range2 with dx = mu_x - px, dy = mu_y - py, t = dx * dx, u = dy * dy, r2 = t + u: six separately rounded
 *              float32 operations, no fused multiply-add; a NaN mean is not visible.  (A 360-degree sensor: no bearing test;
 *              a sensor with a field of view: slam_landmark_evidence_fov_dev below.)
 *   not seen:                              c' = 0
 *   seen, hit_now:                         c' = min(c + hit, cmax), in integers (c = 200, hit = 255 does not wrap)
 *   seen, no hit, visible, c >= miss:      c' = c - miss
 *   seen, no hit, visible, c <  miss:      PRUNED — the five planes of slot l of row i become 0, 0, -1.0f, 0, 0, the bits of a slot
 *                                          that was never used (slam_associate_dev hands it out again), and c' = 0
 *   seen, no hit, not visible:             c' = c
 * d_ev_out[i][l] = c'.  Out of place (d_ev_in != d_ev_out) the padding columns [nlandmarks, ev_stride) of d_ev_out are written
 * 0; in place (d_anc must be NULL) they are left alone.  The padding columns of the map rows, and every plane of a landmark
 * that is not pruned, are never written.  d_stats (may be NULL) is int32 [n][2] = landmarks pruned this frame, landmarks seen
 * after pruning.  Operation order: tests/_evidence_spec.py.
 * slam_evidence_init_dev: d_ev[r][l] = seen ? value : 0 for the nrows rows of d_map (0 <= value <= 255), padding columns 0.
 * SLAM_ERR_INVALID_ARG, nothing launched: hit, miss or cmax outside 1 .. 255, view_range not finite or <= 0, nlandmarks >
 * SLAM_MAX_OBS, assoc_stride, ev_stride or plane_stride < nlandmarks, a gather index with d_ev_in == d_ev_out, a null pointer
 * other than d_anc and d_stats.  SLAM_ERR_NOT_READY: no detections were handed over (ndet == 0 is legal: an observing frame in
 * which every visible seen landmark takes a miss).
 * Timing: both launches are bracketed as SLAM_PROF_PAGES (map bookkeeping), as the association is.  They are counted by
 * slam_evidence_counts (counts[0] evidence launches, counts[1] init launches) and in none of the other counters. */
int slam_landmark_evidence_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                               const float *d_x, const float *d_y, const int32_t *d_anc, int n,
                               const uint8_t *d_assoc, int assoc_stride,
                               const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                               int hit, int miss, int cmax, float view_range, int32_t *d_stats /* [n][2], may be NULL */);
int slam_evidence_init_dev(slam_engine *e, const float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                           int nrows, uint8_t *d_ev, int ev_stride, int value);
int slam_evidence_counts(slam_engine *e, int64_t counts[2]);   /* evidence launches, init launches */
/* LINE OF SIGHT.  The rule above treats the lidar as if it saw through things: a landmark that passes behind a pole or a wall takes
 * a miss in every frame it is hidden, and is pruned with a converged mean and covariance.  The scan itself says what hides what.
 * THE BIN of a sensor-frame point (x, y), for bins a power of two in 32 .. 1024, every step one rounded float32 operation:
 *   ax = |x|, ay = |y|, s = ax + ay; !(s > 0) or s not finite: the point has NO bin; q = ay / s (IEEE division);
 *   p = q (x >= 0, y >= 0), 2 - q (x < 0, y >= 0), 2 + q (x < 0, y < 0), 4 - q (x >= 0, y < 0) — the tests are x < 0 and y < 0, so
 *   -0.0 is not negative; j = (int)(p * (bins / 4)) & (bins - 1) (the product is exact; p == 4 wraps to bin 0).
 * p is the "diamond angle": monotone in the true angle, so bins are contiguous sectors (narrowest on the axes, widest on the
 * diagonals, by a factor of 2).
 * slam_sight_table_dev: THE SIGHT TABLE of the engine's current scan, T[j] = the minimum of r2 = x*x + y*y over the scan's points of
 * bin j, +inf for an empty bin; one launch of one workgroup, into the engine's own buffer.  SLAM_ERR_NOT_READY: no scan;
 * SLAM_ERR_INVALID_ARG: bins.  slam_scan_upload_host / _set_dev drop the table (a stale table is never read).
 * slam_sight_table_get_host: t receives the *bins floats of the table; synchronises.  SLAM_ERR_NOT_READY: no table.
 * slam_landmark_evidence_sight_dev: slam_landmark_evidence_dev with, for the pose (px, py, th = d_th[i]) and dx, dy, r2 of the
 * visibility test:
 *   (s, c) = the update's deterministic sine and cosine of th; zx = c*dx - s*dy, zy = s*dx + c*dy (four products, two sums:
 *   z = R(theta)(w - t)); j = the bin of (zx, zy); near = min(T[(j-1) & (bins-1)], T[j], T[(j+1) & (bins-1)]);
 *   r = sqrtf(r2), g = r - margin (both correctly rounded);
 *   hidden = has a bin && g > 0 && near < g * g                (a NaN anywhere: not hidden)
 * and "seen, no hit, visible" above read "seen, no hit, visible, NOT hidden"; a landmark that is seen, no hit, visible and hidden
 * keeps c.  A hit counts whether the landmark is hidden or not.  d_spared (may be NULL) is int32 [n] = the landmarks spared a
 * miss this way; d_stats as above.  It reads the engine's table (the bins it was built with).  Operation order:
 * tests/_sight_spec.py.  Errors: those of slam_landmark_evidence_dev, a null d_th, a margin that is not finite or <= 0
 * (SLAM_ERR_INVALID_ARG), and SLAM_ERR_NOT_READY without a table.  Both launches are bracketed as SLAM_PROF_PAGES and counted by
 * slam_sight_counts (counts[0] table launches, counts[1] stage launches) — not by slam_evidence_counts.
 * KNOWN LIMIT: a clutter landmark that lies BEHIND a wall is hidden in every frame and is never pruned.  The detector cannot make
 * one (a detection is a piece of the scan); detections handed over from elsewhere can.  d_spared shows it. */
int slam_sight_table_dev(slam_engine *e, int bins);
int slam_sight_table_get_host(slam_engine *e, float *t /* [*bins] out, room for 1024 */, int32_t *bins);
int slam_landmark_evidence_sight_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                     const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                                     const uint8_t *d_assoc, int assoc_stride,
                                     const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                                     int hit, int miss, int cmax, float view_range, float margin,
                                     int32_t *d_stats /* [n][2], may be NULL */, int32_t *d_spared /* [n], may be NULL */);
int slam_sight_counts(slam_engine *e, int64_t counts[2]);      /* table launches, stage launches */
/* A FIELD OF VIEW.  Both rules above treat the sensor as a full circle.  The lidar this project is built around sees 269.5 degrees
 * (1079 beams from -2.351831 rad in steps of 0.004363 rad): a landmark that drifts into the blind quarter behind the robot is
 * "seen, no hit, visible" in every frame, takes a miss per frame and is pruned with a converged mean and covariance — and line of
 * sight does not help, because the bins of the blind quarter are empty and nothing is hidden there.
 * Directions are the DIAMOND ANGLE p of THE BIN above (p in [0, 4], before it is scaled to a bin; no arctangent).
 * slam_fov_bound: a pure host function, the diamond angle of (cosf(angle), sinf(angle)) — the C library's cosine and sine, then the
 * operations of THE BIN; 0 for an angle that is not finite.
 * slam_landmark_evidence_fov_dev: slam_landmark_evidence_sight_dev (use_sight != 0) or slam_landmark_evidence_dev (use_sight == 0)
 * with, for zx, zy as slam_landmark_evidence_sight_dev computes them (the same rotation, the same operation order) and p, "has a
 * bin" of (zx, zy):
 *   in_view = !has a bin || (lo <= hi ? (p >= lo && p <= hi) : (p >= lo || p <= hi))
 * — lo, hi in [0, 4]; a bound itself is in view; a landmark at the sensor is in view; lo > hi is the arc that wraps through p = 4 =
 * 0, the ordinary one for a sensor whose blind sector straddles p = 2; lo = 0, hi = 4 puts everything in view (and the outputs are
 * then, bit for bit, those of the stage it stands in for).  With due = seen, no hit, visible:
 *   due && !in_view: OUTSIDE, c stays;   hidden (use_sight != 0 only) counts only where due && in_view;
 *   a miss is paid where due && in_view && !hidden.   A hit counts whatever the direction.
 * d_outside (may be NULL) is int32 [n] = the landmarks that were due a miss and outside; d_stats and d_spared as above (use_sight ==
 * 0: no table is needed, margin is ignored, d_th is still required, d_spared, if given, is written 0).  Operation order:
 * tests/_fov_spec.py.  Errors: those of slam_landmark_evidence_sight_dev (the margin's and SLAM_ERR_NOT_READY without a table only
 * when use_sight != 0), and SLAM_ERR_INVALID_ARG for a bound that is NaN or outside [0, 4].  The launch is bracketed as
 * SLAM_PROF_PAGES and counted by slam_fov_counts — in no other counter (a table launch still counts in slam_sight_counts[0]). */
float slam_fov_bound(float angle);
int slam_landmark_evidence_fov_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                   const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                                   const uint8_t *d_assoc, int assoc_stride,
                                   const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                                   int hit, int miss, int cmax, float view_range, float margin,
                                   float lo, float hi, int use_sight,
                                   int32_t *d_stats /* [n][2], may be NULL */, int32_t *d_spared /* [n], may be NULL */,
                                   int32_t *d_outside /* [n], may be NULL */);
int slam_fov_counts(slam_engine *e, int64_t *launches);        /* stage launches */
/* MERGING DUPLICATE LANDMARKS: the counterpart of creation.  A gate tight enough for the short axis of an elongated covariance
 * starts a second landmark on a pole that has one; from then on the two slots take turns winning the pole's detection and split
 * its measurements between two half-converged estimates.  Within ONE particle a detection updates exactly one landmark, so two
 * slots on one pole were fed disjoint measurement sets: given the particle's path they are independent estimates of one point,
 * and their product is the posterior — the fusion below is exact per particle, not a heuristic.
 * slam_landmark_merge_dev runs behind the frame's associating update (and behind its evidence stage), IN PLACE on the row the
 * update wrote ([n] rows of the layout of slam_ekf_update_dev, slots l < nlandmarks), with the frame's table d_assoc, K = the
 * engine's current detection count and, optionally, the evidence bytes d_ev:
 *   roles     seen = !(P_xx < 0).  ANCHOR: seen and a_l < K (matched or created this frame).  FREE: seen and not a_l < K.  A table
 *             names a detection at most once, so a particle has at most K <= 64 anchors (of a table that does not, the anchors
 *             behind the 64th in ascending l take no part).  Two anchors are never merged: the detector saw two objects.
 *   choice 1  a free l, over the anchors w in ascending w: d = mu_l - mu_w, S = P_l + P_w element by element, m = d^T S^-1 d in
 *             the operation order of the association's cost with S in the place of P + q I; strict < from +inf — the lowest w on
 *             ties, NaN never wins.  l is a candidate iff 0 <= m <= merge_gate.
 *   choice 2  an anchor absorbs, of the candidates that chose it, the one with the smallest m (the lowest l on ties) — ONE per
 *             frame; the others wait for the next frame.
 *   fusion    the general-covariance update (slam_ekf_update_aniso_dev's arithmetic) of the anchor with mu_l as the observed
 *             point and P_l as the noise: mu' = mu_l - P_l S^-1 (mu_l - mu_w), P' = (det P_w * P_l + det P_l * P_w) / det S.
 *             No likelihood term.
 *   guard     REFUSED — counted, nothing written — unless the five fused values are finite, P'_xx > 0, P'_yy > 0 and
 *             P'_xx P'_yy - P'_xy^2 > 0 in float32: a merge never writes a covariance that is negative or not finite into an
 *             anchor (P_xx < 0 would silently turn it into an unused slot).
 *   result    the anchor takes the fused values; the five planes of slot l become 0, 0, -1, 0, 0 (a slot that was never used,
 *             as in pruning); with evidence c_w' = min(c_w + c_l, cmax) in integers and c_l' = 0.  Padding columns are never
 *             written.
 * d_stats (may be NULL) is int32 [n][3] = merged, refused, seen after the stage.  Operation order: tests/_merge_spec.py.
 * KNOWN LIMITS: one absorption per anchor and frame; anchors are never merged with anchors (two slots that were both matched
 * or created this frame stay two); rows on one GPU only.
 * Errors, nothing launched: SLAM_ERR_INVALID_ARG for a merge_gate that is not finite or <= 0, plane_stride or assoc_stride <
 * nlandmarks, row_stride < 5 * plane_stride, nlandmarks > SLAM_MAX_OBS, n < 0, a null d_map or d_assoc, and — when d_ev is given —
 * ev_stride < nlandmarks or cmax outside 1 .. 255 (d_ev == NULL: ev_stride and cmax are not read); SLAM_ERR_NOT_READY when no
 * detections were handed over.  No detections in the frame (K = 0) is legal: no anchors, nothing happens, seen is counted.  The
 * launch is bracketed as SLAM_PROF_PAGES and counted by slam_merge_count — in no other counter. */
int slam_landmark_merge_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks, int n,
                            const uint8_t *d_assoc, int assoc_stride,
                            uint8_t *d_ev /* may be NULL */, int ev_stride, int cmax, float merge_gate,
                            int32_t *d_stats /* [n][3], may be NULL */);
int slam_merge_count(slam_engine *e, int64_t *launches);       /* stage launches */
/* WHAT THE ASSOCIATION LEAVES UNEXPLAINED.  The associating update's log-likelihood (slam_ekf_update_assoc_dev and its siblings)
 * sums one term per MATCHED pair, -m/2 - log det S / 2 - log 2 pi: a log DENSITY in 1/m^2.  A detection that starts a landmark, one
 * that is dropped (between the two gates, or because no slot is left) and a landmark in view that took no detection contribute
 * nothing — an implicit, dimensionless 0, so which particle the filter prefers depends on the unit of length: for P = p I under
 * q = meas_var the matched term is -m/2 - log(2 pi (p + q)), negative for EVERY m once p + q > 1 / (2 pi) = 0.159 m^2, and a
 * particle whose pose is wrong enough that every detection misses the gate then outweighs one that matches all of them.  The
 * remedy is FastSLAM with unknown data association: a constant log-likelihood for a new feature, a log clutter density for an
 * unexplained detection and log(1 - P_D) for a missed landmark.
 * THE MISS COUNT.  The _missed siblings of the three evidence stages are those stages — the same kernels, launch counters, errors,
 * map, evidence bytes and stats — with one more optional output: d_missed int32 [n] = the slots of particle i the stage scored as
 * a miss in the form it runs (plain, line of sight, field of view, both): the slots whose evidence byte it lowered or whose
 * landmark it pruned.  A landmark spared by line of sight or outside the arc is no miss.  d_missed == NULL: exactly the call
 * without the suffix (which is how those are implemented).
 * slam_assoc_weight_dev: one thread per particle, with created_i = d_stats[3 i + 1] and dropped_i = d_stats[3 i + 2] (the stats of
 * the association: matched, created, dropped) and missed_i = d_missed[i] (NULL: 0), every line one rounded float32 operation
 * (tests/_assoc_weight_spec.py), the counts converted exactly:
 *   t = created * log_new;  u = dropped * log_clutter;  t = t + u;  u = missed * log_miss;  t = t + u;  ll[i] = ll[i] + t
 * in place on d_loglik — NULL: the engine's log-likelihood buffer, what slam_logweight_ekf_dev consumes (SLAM_ERR_NOT_READY unless
 * the last landmark update on this engine was of n particles); d_terms (may be NULL) receives t.  The three constants must be
 * finite and <= 0 (-0.0 is), else SLAM_ERR_INVALID_ARG and nothing is launched; likewise for n < 0 or a null d_stats.  A sum that
 * overflows is -inf, as the specification's is.  Bracketed as SLAM_PROF_PAGES and counted by slam_assoc_weight_count — in no other
 * counter. */
int slam_landmark_evidence_missed_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                      const float *d_x, const float *d_y, const int32_t *d_anc, int n,
                                      const uint8_t *d_assoc, int assoc_stride,
                                      const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                                      int hit, int miss, int cmax, float view_range, int32_t *d_stats /* [n][2], may be NULL */,
                                      int32_t *d_missed /* [n], may be NULL */);
int slam_landmark_evidence_sight_missed_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                            const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                                            const uint8_t *d_assoc, int assoc_stride,
                                            const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                                            int hit, int miss, int cmax, float view_range, float margin,
                                            int32_t *d_stats /* [n][2], may be NULL */, int32_t *d_spared /* [n], may be NULL */,
                                            int32_t *d_missed /* [n], may be NULL */);
int slam_landmark_evidence_fov_missed_dev(slam_engine *e, float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                                          const float *d_x, const float *d_y, const float *d_th, const int32_t *d_anc, int n,
                                          const uint8_t *d_assoc, int assoc_stride,
                                          const uint8_t *d_ev_in, uint8_t *d_ev_out, int ev_stride,
                                          int hit, int miss, int cmax, float view_range, float margin,
                                          float lo, float hi, int use_sight,
                                          int32_t *d_stats /* [n][2], may be NULL */, int32_t *d_spared /* [n], may be NULL */,
                                          int32_t *d_outside /* [n], may be NULL */, int32_t *d_missed /* [n], may be NULL */);
int slam_assoc_weight_dev(slam_engine *e, const int32_t *d_stats /* [n][3] */, const int32_t *d_missed /* [n], may be NULL */, int n,
                          float log_new, float log_clutter, float log_miss,
                          float *d_loglik /* [n]; NULL: the engine's buffer */, float *d_terms /* [n], may be NULL */);
int slam_assoc_weight_count(slam_engine *e, int64_t *launches);   /* stage launches */
/* LOCALISATION IN A KNOWN MAP (specification: tests/_localise_spec.py).  ONE landmark map every particle
 * shares, which nothing changes: d_map is float32 [5][plane_stride], planes mx, my, P_xx, P_xy, P_yy as in a row, 1 <= nlandmarks
 * <= SLAM_MAX_OBS, plane_stride >= nlandmarks; a slot with P_xx < 0 holds no landmark.  With meas_var * I noise S^-1 = (P + meas_var I)^-1 and
 * 0.5 log det S do not depend on the particle:
 * slam_known_map_prepare_dev works them out once per map (one launch) into d_prepared, float32 [6][plane_stride] = mx, my, i00,
 * i01, i11, hl — the operations of the landmark update, so the bits the specification computes per particle; a slot without a
 * landmark, and the padding behind nlandmarks, get a NaN mx and never become candidates.  The caller guarantees P + meas_var I
 * positive definite for every landmark (slam_pf_known_map_set checks it).
 * slam_localise_dev (one launch): every particle associates the engine's current detections (uploaded, set or made by the
 * detector; K = 0 is legal: loglik = +0, stats = 0) with the prepared map exactly as slam_associate_dev(create = 0, new_gate = gate)
 * would with a row that holds it — each landmark its cheapest detection, each detection the cheapest landmark that chose it, 0 <=
 * m <= gate, the lowest k and the lowest l on ties, NaN never wins — and leaves the log-likelihood slam_ekf_update_assoc_dev would
 * leave under that table (the matched pairs' terms, summed in its order) in d_loglik (NULL: the engine's buffer, what
 * slam_logweight_ekf_dev and slam_assoc_weight_dev consume).  d_stats int32 [n][3] = matched, 0, K - matched.  d_assoc (may be
 * NULL: no table is written) is uint8 [n][assoc_stride >= nlandmarks] as slam_associate_dev writes it.  No row is read and none is
 * written.  SLAM_ERR_INVALID_ARG: nlandmarks outside 1 .. SLAM_MAX_OBS, plane_stride or (with d_assoc) assoc_stride < nlandmarks,
 * a gate that is not finite and > 0, n < 0, a null pointer other than d_assoc / d_loglik.  SLAM_ERR_NOT_READY: no detections.
 * Out of scope: one 2x2 noise for all detections as a form of its own (attach the same Q to every detection of
 * slam_localise_detcov_dev), any change of the map, K > 64.
 * UNDER A COVARIANCE PER DETECTION (specification: tests/_localise_detcov_spec.py): slam_localise_detcov_dev (one launch) is
 * slam_localise_dev under S = P + R_w(theta_i, k) of the engine's current detections AND THEIR COVARIANCES
 * (slam_detections_cov_upload_host / _set_dev, slam_detect_scan_noise_dev) — exactly what slam_associate_detcov_dev(create = 0,
 * new_gate = gate) and the log-likelihood of slam_ekf_update_assoc_detcov_dev give on rows that each hold the map.  S^-1 depends on
 * the particle and the detection, so nothing is prepared: d_map is the map as it was given, float32 [5][plane_stride]; a slot with
 * P_xx < 0, and the padding behind nlandmarks, never become candidates.  The caller guarantees P positive semi-definite for every
 * landmark (slam_pf_known_map_detcov_set checks it; every Q_k is positive definite).  d_stats, d_assoc, d_loglik and the refused
 * arguments as for slam_localise_dev; SLAM_ERR_NOT_READY also when the detections carry no covariances.
 * slam_localise_detcov_count: its launches (in no other counter).
 * THE LANDMARKS IN VIEW THAT NO DETECTION MATCHED (specification: tests/_localise_miss_spec.py): slam_localise_miss_dev and
 * slam_localise_detcov_miss_dev are the two stages above — d_loglik, d_stats and d_assoc bit for bit — whose ONE launch also
 * counts, per particle, what the map says the pose should have seen, under the evidence stage's own predicate
 * (slam_landmark_evidence_fov_dev) with every landmark the frame's matching hit taken as hit: a landmark that is seen, is no
 * detection's match and lies within view->view_range of the pose is
 *   outside  its sensor-frame direction lies outside the arc [view->lo, view->hi] of the diamond angle (slam_fov_bound; lo > hi: the
 *            arc through 4 = 0; 0, 4: the whole circle, nothing is outside);
 *   spared   in the arc and hidden behind what the scan hit (view->sight != 0: the engine's current sight table,
 *            slam_sight_table_dev, and view->margin; else nothing is hidden);
 *   missed   in the arc and not hidden.
 * d_missed int32 [n]; d_spared and d_outside likewise, each may be NULL.  The log-likelihood does not contain the misses:
 * slam_assoc_weight_dev(d_stats, d_missed, .., log_miss) adds their term, as in the mapping pipeline.  A pose that is not finite
 * counts nothing.  SLAM_ERR_INVALID_ARG besides the stage's own: a null view or d_missed, a view_range that is not finite and > 0,
 * bounds outside [0, 4], with sight a margin that is not finite and > 0.  SLAM_ERR_NOT_READY besides the stage's own: sight and no
 * sight table made since the current scan.  slam_localise_miss_count: the launches of the two (in no other counter). */
typedef struct {
    float view_range;
    float lo, hi;   /* diamond bounds; 0, 4: the whole circle */
    int sight;      /* 0: off; else the engine's current sight table is read */
    float margin;
} slam_localise_view;
int slam_known_map_prepare_dev(slam_engine *e, const float *d_map /* [5][plane_stride] */, int plane_stride, int nlandmarks,
                               float meas_var, float *d_prepared /* [6][plane_stride] */);
int slam_localise_dev(slam_engine *e, const float *d_prepared, int plane_stride, int nlandmarks,
                      const float *d_x, const float *d_y, const float *d_th, int n, float gate,
                      uint8_t *d_assoc /* may be NULL */, int assoc_stride, int32_t *d_stats /* [n][3] */,
                      float *d_loglik /* NULL: the engine's buffer, what slam_logweight_ekf_dev consumes */);
int slam_localise_counts(slam_engine *e, int64_t counts[2]);        /* prepare launches, stage launches */
int slam_localise_detcov_dev(slam_engine *e, const float *d_map /* [5][plane_stride] */, int plane_stride, int nlandmarks,
                             const float *d_x, const float *d_y, const float *d_th, int n, float gate,
                             uint8_t *d_assoc /* may be NULL */, int assoc_stride, int32_t *d_stats /* [n][3] */,
                             float *d_loglik /* NULL: the engine's buffer, what slam_logweight_ekf_dev consumes */);
int slam_localise_detcov_count(slam_engine *e, int64_t *launches);  /* stage launches */
int slam_localise_miss_dev(slam_engine *e, const float *d_prepared, int plane_stride, int nlandmarks,
                           const float *d_x, const float *d_y, const float *d_th, int n, float gate,
                           uint8_t *d_assoc /* may be NULL */, int assoc_stride, int32_t *d_stats /* [n][3] */,
                           float *d_loglik /* NULL: the engine's buffer */, const slam_localise_view *view,
                           int32_t *d_missed /* [n] */, int32_t *d_spared /* may be NULL */, int32_t *d_outside /* may be NULL */);
int slam_localise_detcov_miss_dev(slam_engine *e, const float *d_map /* [5][plane_stride] */, int plane_stride, int nlandmarks,
                                  const float *d_x, const float *d_y, const float *d_th, int n, float gate,
                                  uint8_t *d_assoc /* may be NULL */, int assoc_stride, int32_t *d_stats /* [n][3] */,
                                  float *d_loglik /* NULL: the engine's buffer */, const slam_localise_view *view,
                                  int32_t *d_missed /* [n] */, int32_t *d_spared /* may be NULL */, int32_t *d_outside /* may be NULL */);
int slam_localise_miss_count(slam_engine *e, int64_t *launches);    /* launches of the two miss forms */
/* RESEEDING THE CLOUD FROM WHAT THE LIDAR SEES (specification: tests/_reseed_spec.py reseed): sensor-resetting
 * localisation.  If detection k is landmark j, the robot stands on a circle of radius |z_k| around landmark j and its heading is
 * fixed by where on the circle it stands; drawing j, k and the heading gives a one-dimensional family per (j, k) instead of the
 * volume a cloud scattered over x, y and theta has to fill.  slam_pose_reseed_dev (one launch, no pose passes through the host)
 * replaces a chosen fraction of n slots by such proposals over the engine's current detections (uploaded, set or made by the
 * detector; K of them) and a known map as it was given, d_map float32 [5][plane_stride], P_xx < 0: the slot holds no landmark.
 * Slot i, gid = first_id + i:
 *     r = philox4x32_10(lo(gid), hi(gid), frame, 2, key = lo(seed), hi(seed))     (stream 2; 0 and 1 are motion and resample)
 *     chosen iff (uint64)r[0] < thr,   thr = floor((double)fraction * 2^32) held in 64 bits (fraction == 1: 2^32, every slot)
 *     j = umulhi(r[1], nlandmarks),  k = umulhi(r[2], K),  theta = 6.2831853072f * ((float)(r[3] >> 8) * 2^-24)
 *     (s, c) = the specified sine and cosine of theta; then, every product and sum one binary32 rounding in this order — the
 *     update's w = p + H^T z read backwards:
 *         t = c * zx_k;  v = s * zy_k;  t = t + v;  x' = mx_j - t;
 *         t = c * zy_k;  v = s * zx_k;  t = t - v;  y' = my_j - t;     th' = theta
 * A chosen slot whose slot j holds no landmark is not replaced.  A slot that is not replaced copies (x, y, th)[d_anc[i]] (d_anc
 * NULL: i) — the pending resample rides along.  No jitter is added: the next frame's motion sample spreads the proposals.
 * d_flag (may be NULL) uint8 [n]: 1 replaced, 2 chosen but not replaced, 0 otherwise; counts = {replaced, chosen but not replaced},
 * exact; the call synchronises to return them.  In place (every out array is its in array) is allowed exactly when d_anc is NULL;
 * any other overlap of an in and an out array is SLAM_ERR_INVALID_ARG, as are n <= 0, nlandmarks <= 0, plane_stride < nlandmarks,
 * a fraction that is not in (0, 1] (or not a number) and a null pointer other than d_anc / d_flag.  SLAM_ERR_NOT_READY: no
 * detections were handed over.  K == 0: SLAM_OK, nothing is written, counts 0.  slam_pose_reseed_count: its launches (in no other
 * counter).  Out of scope: deciding when to reseed.  Proposals from detection pairs: slam_pose_reseed_pairs_dev below. */
int slam_pose_reseed_dev(slam_engine *e, const float *d_map /* [5][plane_stride] */, int plane_stride, int nlandmarks,
                         const float *d_x_in, const float *d_y_in, const float *d_th_in, const int32_t *d_anc /* NULL: identity */,
                         float *d_x_out, float *d_y_out, float *d_th_out, int n, int64_t first_id, uint64_t seed, uint32_t frame,
                         float fraction, uint8_t *d_flag /* may be NULL */, int32_t counts[2]);
int slam_pose_reseed_count(slam_engine *e, int64_t *launches);
/* RESEEDING FROM DETECTION PAIRS (specification: tests/_reseed_pair_spec.py reseed_pairs): one detection on one
 * landmark leaves the heading to be drawn blind; two detections k1, k2 on two landmarks j1, j2 fix the pose completely, and the
 * pairing is checked before the proposal is made, because |z_k2 - z_k1| must be |m_j2 - m_j1|.  j1, k1 and k2 are drawn, j2 is
 * searched for in the map (O(nlandmarks) per proposal, done by the wavefront) and drawn among the landmarks that fit.  Map,
 * detections, in/out arrays, d_anc, first_id, seed, frame and fraction as slam_pose_reseed_dev.  tol >= 0, min_sep > tol, both
 * finite; min_sep2 = min_sep * min_sep rounded once.  Every product, sum, difference, quotient and square root below is one
 * binary32 rounding, in this order.  Slot i, gid = first_id + i:
 *     rA = philox4x32_10(lo(gid), hi(gid), frame, 2, key)   the stream and threshold of slam_pose_reseed_dev: chosen iff
 *          (uint64)rA[0] < thr, so both calls choose the same slots
 *     j1 = umulhi(rA[1], nlandmarks),  k1 = umulhi(rA[2], K),  k2 = umulhi(rA[3], K - 1);  k2 += (k2 >= k1)
 *     rB = philox4x32_10(lo(gid), hi(gid), frame, 3, key)   stream 3: rB[0] picks the partner, the other words are unused
 * and for a chosen slot, in this order:
 *     1. ax = zx_k2 - zx_k1;  ay = zy_k2 - zy_k1;  t = ax * ax;  u = ay * ay;  dz2 = t + u.  !(dz2 >= min_sep2) (a NaN as well):
 *        the detections are too close to fix a heading — flag 3.
 *     2. P_xx[j1] < 0: slot j1 holds no landmark — flag 2.
 *     3. dz = sqrt(dz2);  lo = dz - tol;  hi = dz + tol;  lo2 = lo * lo;  hi2 = hi * hi.  Landmark j is a PARTNER iff j != j1,
 *        !(P_xx[j] < 0), and with bx = mx_j - mx_j1; by = my_j - my_j1; t = bx * bx; u = by * by; dm2 = t + u:
 *        dm2 > 0 && lo2 <= dm2 && dm2 <= hi2 (squared distances only; both bounds inclusive).  cnt = the number of partners;
 *        cnt == 0 — flag 4.
 *     4. c = umulhi(rB[0], cnt), j2 = the c-th partner in ascending j (so the result does not depend on how the search is
 *        scheduled), b = m_j2 - m_j1 as above;
 *            t = bx * ay;  u = by * ax;  cr = t - u;   t = ax * bx;  u = ay * by;  dt = t + u;
 *            theta = det_atan2(cr, dt);  theta < 0: theta = theta + 6.2831853072f     (the angle of a less the angle of b: the
 *            update's world offset of a detection is (c zx + s zy, c zy - s zx))
 *        (s, c) = the specified sine and cosine of theta, and (x', y') from (m_j1, z_k1, s, c) exactly as slam_pose_reseed_dev
 *        forms them; th' = theta — flag 1.
 *     det_atan2(y, x): hi = max(|x|, |y|), lo = the other (swapped iff |y| > |x|);  t = lo / hi;  t > 0.4142135623730950f:
 *        y0 = 0.7853981634f, t = (t - 1) / (t + 1), else y0 = 0;  z = t * t;
 *        p = 8.05374449538e-2f * z; p = p - 1.38776856032e-1f; p = p * z; p = p + 1.99777106478e-1f; p = p * z;
 *        p = p - 3.33329491539e-1f; p = p * z; p = p * t; p = p + t;  r = y0 + p;  swapped: r = 1.5707963268f - r;
 *        x < 0: r = 3.1415926536f - r;  y < 0: r = -r.  (0, 0) cannot arise: min_sep > tol >= 0 and dm2 > 0 keep a and b non-zero.
 * A slot that is not replaced copies (x, y, th)[d_anc[i]] (d_anc NULL: i).  d_flag (may be NULL) uint8 [n]: the flags above, 0 not
 * chosen; counts = {replaced, j1 empty, too close, no partner}, exact; the call synchronises to return them.
 * Every refusal of slam_pose_reseed_dev applies; SLAM_ERR_INVALID_ARG also for !(tol >= 0), !(min_sep > tol), a non-finite value of
 * either, and nlandmarks < 2.  K < 2: SLAM_OK, nothing is written, counts 0.  slam_pose_reseed_pairs_count: its launches (in no
 * other counter).  Out of scope: a fallback to single-detection proposals in the same call (call slam_pose_reseed_dev), searching
 * all pairs of landmarks, deciding when to reseed. */
int slam_pose_reseed_pairs_dev(slam_engine *e, const float *d_map /* [5][plane_stride] */, int plane_stride, int nlandmarks,
                               const float *d_x_in, const float *d_y_in, const float *d_th_in, const int32_t *d_anc /* NULL: identity */,
                               float *d_x_out, float *d_y_out, float *d_th_out, int n, int64_t first_id, uint64_t seed, uint32_t frame,
                               float fraction, float tol, float min_sep, uint8_t *d_flag /* may be NULL */, int32_t counts[4]);
int slam_pose_reseed_pairs_count(slam_engine *e, int64_t *launches);
/* THE DETECTOR: the detections of a frame made on the device from the engine's current scan (slam_scan_upload_host / _set_dev),
 * P = nbeams points in scan order — what fe_clean left, so a removed beam leaves no hole and the rule uses distances only, never
 * beam angles.  With jump2 = jump * jump, guard2, width2 and range2 likewise (each rounded once to float32), and every step below
 * one separately rounded float32 operation:
 *   1. per point b: r2_b = x*x + y*y; g_b = dx*dx + dy*dy against point b - 1 (g_0: against point P - 1 with wrap, else +inf);
 *      break_b = !(g_b <= jump2) (a NaN breaks);
 *   2. every break f starts a SEGMENT: the points from f up to, excluding, the next break — cyclic through P - 1 into 0 with
 *      wrap; without it the walk ends at P - 1, and a segment that holds point 0 or point P - 1 is rejected (cut by the field of
 *      view).  m = its point count, e = its last point.  A scan without a break has no segment;
 *   3. a segment is ACCEPTED iff (a) min_points <= m <= max_points, (b) dx = x_e - x_f, dy alike, dx*dx + dy*dy <= width2, (c) it
 *      is occluded at neither end — left, with p the point before f: g_f <= guard2 && r2_p < r2_f; right, with q the point after
 *      e: g_q <= guard2 && r2_q < r2_e (something close to an end and in front of it may hide part of the object) — and (d) its
 *      centroid zx = sx / (float)m, zy alike (sx = x_f, then + x over the other points in segment order; IEEE division) has
 *      zx*zx + zy*zy <= range2.  NaN and inf pass none of the tests: every detection is finite;
 *   4. the accepted segments in ascending f, the first SLAM_MAX_DETECTIONS of them, are the engine's current detections:
 *      zx[k] | zy[k] in the engine's own buffer, no copy through the host.  d_stats (may be NULL) is int32 [4] = segments,
 *      accepted, written (= ndet), 0.  Operation order: tests/_detect_spec.py.
 * slam_detect_scan_dev is asynchronous: the count of the detections is PENDING afterwards — the kernel leaves it in mapped host
 * memory, and slam_associate_dev, slam_ekf_update_assoc_dev and slam_landmark_evidence_dev pick it up first thing (a wait on a
 * flag word: no copy, no stream synchronisation); with nothing pending they do what they did.  slam_detections_upload_host /
 * _set_dev replace the detections and end the pending state.  SLAM_ERR_INVALID_ARG, nothing launched: a length that is not
 * finite and > 0, guard < jump, not 1 <= min_points <= max_points <= SLAM_DETECT_MAX_POINTS, wrap not 0 or 1, a null pointer other
 * than d_stats.  SLAM_ERR_NOT_READY: no scan.  Timing: bracketed as SLAM_PROF_PAGES, as the association is.  Counted by
 * slam_detect_count, and in no other counter.
 * slam_detections_get_host: the engine's current detections whatever their origin — zx and zy hold SLAM_MAX_DETECTIONS values
 * each, the first *ndet the detections, the rest 0 (after slam_detect_scan_dev: the block as the kernel left it); synchronises.
 * SLAM_ERR_NOT_READY: none were handed over or made. */
enum { SLAM_DETECT_MAX_POINTS = 64 };
typedef struct {
    float jump;          /* a gap between neighbouring points above this breaks the scan [m] */
    float guard;         /* a nearer neighbour within this of a segment's end occludes it [m]; >= jump */
    float max_width;     /* first to last point of a segment [m] */
    float max_range;     /* of the centroid [m] */
    int32_t min_points;  /* 1 <= min_points <= max_points <= SLAM_DETECT_MAX_POINTS */
    int32_t max_points;
    int32_t wrap;        /* 1: a 360-degree scan, point 0 follows point P - 1; 0: the ends are the edge of the field of view */
} slam_detect_params;
void slam_detect_params_default(slam_detect_params *p);   /* 0.3, 1.0, 0.5, 20.0, 3, 40, 1 */
int slam_detect_scan_dev(slam_engine *e, const slam_detect_params *params, int32_t *d_stats /* [4], may be NULL */);
int slam_detect_count(slam_engine *e, int64_t *launches);
/* THE DETECTOR, FITTED: a pole has a known nominal radius, and with it the centre of the circle through a segment's points has a
 * closed form that uses every point.  With c the centroid, s2 the mean squared distance of the m points to it and C the centre,
 * sum (p_i - c) = 0 gives mean |p_i - C|^2 = s2 + |c - C|^2; on the circle the left side is radius^2, so C lies
 * sqrt(radius^2 - s2) from c, along the line of sight through c.  slam_detect_scan_fit_dev is slam_detect_scan_dev (fit == NULL:
 * exactly that, bit for bit and launch for launch) with, behind step 3(d) — whose test of the centroid stays — for every segment,
 * rho2 = radius * radius, lim = rho2 + spread_tol * spread_tol and range2 rounded once, every step one float32 operation:
 *   (e) q = 0, then for the points in segment order du = x - cx, dv = y - cy, q = q + (du*du + dv*dv); s2 = q / (float)m;
 *       s2 <= lim and cx*cx + cy*cy > 0, or the segment is REJECTED BY THE SHAPE TEST: more spread out than a pole can be (a flat
 *       piece of wall wider than about 3.46 radius), or its centroid on the sensor;
 *   (f) t = max(rho2 - s2, 0); d = sqrt(t); n = sqrt(cx*cx + cy*cy); zx = cx + d * (cx / n), zy alike (correctly rounded sqrt and
 *       division); accepted iff zx*zx + zy*zy <= range2.
 * d_stats[3] counts the segments the shape test rejected (0 without a fit).  Operation order: tests/_detect_fit_spec.py.
 * SLAM_ERR_INVALID_ARG, nothing launched: as slam_detect_scan_dev, or a radius that is not finite and > 0, a spread_tol that is
 * not finite and >= 0.  Counted by slam_detect_count like every detector launch, and by slam_detect_fit_count when a fit ran. */
typedef struct {
    float radius;       /* the poles' nominal radius [m] */
    float spread_tol;   /* what the shape test allows beyond it: s2 <= radius^2 + spread_tol^2 [m] */
} slam_detect_fit;
void slam_detect_fit_default(slam_detect_fit *f);   /* 0.1, 0.0 */
int slam_detect_scan_fit_dev(slam_engine *e, const slam_detect_params *params, const slam_detect_fit *fit /* NULL: the centroid */,
                             int32_t *d_stats /* [4], may be NULL */);
int slam_detect_fit_count(slam_engine *e, int64_t *launches);   /* launches that ran the fit; slam_detect_count counts all */
int slam_detections_get_host(slam_engine *e, float *zx, float *zy, int32_t *ndet);
/* THE DETECTOR'S NOISE MODEL.  A lidar measures range well and bearing less well, and the cross-beam error grows with range.
 * slam_detect_scan_noise_dev is slam_detect_scan_fit_dev (noise == NULL: exactly that call, bit for bit and launch for launch)
 * and, with a model, gives every detection (zx, zy) that passed its range test the covariance the per-detection stages read
 * (slam_associate_detcov_dev): r2 = zx zx + zy zy, rho = sqrt(r2), u = (zx, zy) / rho, a = range_var, b = bearing_var r2 +
 * lateral_var, Q = a u u^T + b v v^T with v normal to u: qxx = a ux^2 + b uy^2, qxy = (a - b) ux uy, qyy = a uy^2 + b ux^2 — every
 * step one rounded float32 operation, in the order of tests/_detect_noise_spec.py.  A detection with r2 == 0, or whose Q fails
 * the rule of slam_detections_cov_upload_host (cancellation in its determinant at extreme a : b), is NO detection; the cap at
 * SLAM_MAX_DETECTIONS applies after this rule.  d_stats (may be NULL) is then int32[6]: the four words of
 * slam_detect_scan_fit_dev (accepted and written count what passed this rule too), the number dropped by it, 0.
 * SLAM_ERR_INVALID_ARG, nothing launched: as slam_detect_scan_fit_dev, or range_var not finite and > 0, bearing_var [rad^2] or
 * lateral_var not finite and >= 0, bearing_var + lateral_var not > 0.  One launch of one workgroup; counted by slam_detect_count
 * (and slam_detect_fit_count with a fit) and, with a model, by slam_detect_noise_count too. */
typedef struct slam_detect_noise {
    float range_var;     /* variance along the line of sight [m^2] */
    float bearing_var;   /* variance of the bearing [rad^2]: bearing_var * r^2 across the line of sight */
    float lateral_var;   /* range-independent variance across the line of sight [m^2] */
} slam_detect_noise;
int slam_detect_scan_noise_dev(slam_engine *e, const slam_detect_params *params, const slam_detect_fit *fit /* NULL: the centroid */,
                               const slam_detect_noise *noise /* NULL: slam_detect_scan_fit_dev */, int32_t *d_stats /* [6] with noise, may be NULL */);
int slam_detect_noise_count(slam_engine *e, int64_t *launches);
/* The FRONT of a frame of a single-GPU slam_pf session on rows — motion sample + scan-match score (FastMatch's inner loop,
 * main.c:459-518, for every particle) and the out-of-place landmark update — goes out as ONE launch whose scoring and
 * updating workgroups are dealt out interleaved: the scorer's gathers (texture addresser, L2) run in the shadow of the
 * update's row stores (HBM).  Same bits as the two launches.  on = 1 (the initial state) / 0: two launches (stage timers,
 * measurements).  Paged sessions, gated sessions on rows, sharded sessions
 * on rows, short rows and small populations always take the two launches (a sharded session on the split layout fuses the
 * score with the update of the groups whose ancestors are local), and so does every frame while SLAM_PROF_SCORE is being timed
 * (slam_profile_enable: a fused launch is bracketed as SLAM_PROF_EKF), and every frame of a session that refines its poses
 * (slam_pf_refine_set: the update must read the REFINED poses, the fused launch would work out the unrefined sample again).
 * slam_frame_fusion_count: fused launches of this engine so far. */
int slam_frame_fusion_set(slam_engine *e, int on);
int slam_frame_fusion_count(slam_engine *e, int64_t *launches);
/* SURVIVOR ROWS.  On the split layout the fused front launch of a single-GPU session that resamples every frame
 * (resample_ess_frac == 0) writes no mean row: the next frame reads a row only through the resample index, and most
 * particles leave no offspring.  One launch behind the resample writes the rows of the particles it kept, from the inputs
 * the frame started from, bit for bit what the front launch would have written.  Whatever else looks at mean rows
 * (slam_pf_device_view and its kin, slam_pf_get_map_host, a change of layout, a frame that does not qualify) first gets
 * them all written by one more launch, so no result depends on the switch.  on = 1 (the initial state; the environment
 * variable SLAM_SURVIVOR_ROWS=0 makes 0 the initial state of engines created afterwards) / 0: every frame writes every row.
 * Neither launch counts in slam_ekf_form_counts or slam_frame_fusion_count; both are bracketed as SLAM_PROF_MATERIALISE. */
int slam_survivor_rows_set(slam_engine *e, int on);
/* Which instantiation the LAST fused front launch of this engine was (tests pin the kernel at the shapes its numbers are
 * quoted on and say which one they pinned): info[0] = particles per updating wavefront (2 or 4; 2, 4 or 8 on the split
 * layout), info[1] = lanes per pose of its scoring workgroups (4 below 131 072 particles, else 1); both 0 before the first
 * fused launch. */
int slam_frame_front_last(slam_engine *e, int32_t info[2]);
/* The in-place update (d_map_in == d_map_out: frames that keep their population, slam_resample_gate_set) also has two
 * kernels with the SAME bits: whole rows in batches of 128 landmarks, and the observed landmarks only, from a list
 * the engine compacts out of the observation table once per table (nlandmarks <= 65536).  form = -1 (initial): the
 * second whenever the last list built for this nlandmarks held at most nlandmarks / 4 observations; 0 / 1 force the
 * first / second (tests, measurements).
 * counts[0] / counts[1]: in-place launches so far of the first / second. */
int slam_ekf_inplace_form_set(slam_engine *e, int form);
int slam_ekf_inplace_form_counts(slam_engine *e, int64_t counts[2]);

/* A11: logw[i] = loglik[i] - score[i] * score_gain  (either input may be NULL = 0) and
 * *d_max = max_i logw[i] (float, device).  Then, with the GLOBAL maximum m (after an all-reduce MAX
 * over shards): wq[i] = (uint64) (exp_det(logw[i] - m) * 2^32)  and  *d_sum = sum(wq)  (exact
 * integer, hence independent of summation order and sharding). */
int slam_logweight_dev(slam_engine *e, const float *d_score, const float *d_loglik, float score_gain, int n,
                       float *d_logw, float *d_max);
int slam_quantise_weights_dev(slam_engine *e, const float *d_logw, const float *d_max, int n, uint64_t *d_wq,
                              uint64_t *d_sum);
/* slam_logweight_dev with loglik = the log-likelihood of the last slam_ekf_update_dev(…, n, …) call on this
 * engine, taken from wherever that call left it (see there). */
int slam_logweight_ekf_dev(slam_engine *e, const float *d_score, float score_gain, int n, float *d_logw,
                           float *d_max);

/* Fused form of the two stages above + the prefix sum below, for the frame loop: weights are quantised and
 * scanned in one pass and never stored; the engine keeps the scan for slam_offspring_from_scan_dev.
 *   d_max  NULL on a single GPU = use the maxima the preceding slam_logweight_dev(…, n, …, d_max = NULL or
 *          not) left inside the engine; on several GPUs pass the all-reduced maximum.
 *   d_sum  shard total written to the device for the all-gather between GPUs; may be NULL on one GPU.
 * slam_logweight_dev accepts d_max == NULL (the global maximum is then not materialised). */
int slam_quantise_scan_dev(slam_engine *e, const float *d_logw, const float *d_max, int n, uint64_t *d_sum);
/* = slam_offspring_offsets_dev on the scan kept by slam_quantise_scan_dev; d_total may be NULL on a
 * single GPU (the grand total is then the shard total, derived inside the kernel). */
int slam_offspring_from_scan_dev(slam_engine *e, int n, const uint64_t *d_base, const uint64_t *d_total,
                                 uint64_t seed, uint32_t frame, int64_t n_total, int32_t *d_first);
/* Several GPUs: base offset and grand total derived inside the kernel from the all-gathered shard totals
 * (d_shard_totals[world], what slam_quantise_scan_dev wrote to d_sum on every rank). */
int slam_offspring_from_scan_sharded_dev(slam_engine *e, int n, const uint64_t *d_shard_totals, int rank, int world,
                                         uint64_t seed, uint32_t frame, int64_t n_total, int32_t *d_first);

/* Resample gate (ESS-gated resampling).  ess_frac in (0, 1): a frame resamples only when the effective sample size
 * of its weights is below ess_frac * N; anything else (the initial state): every frame resamples.  The ESS is taken
 * on 16-bit weights v = wq >> 16, ESS = (sum v)^2 / sum v^2, and compared in exact integer arithmetic
 * ((sum v)^2 * 65536 < round(ess_frac * 65536) * N * sum v^2), so the verdict is the same for any sharding.
 * With a gate set, on this engine:
 *  - slam_quantise_scan_dev also keeps carry[i] = logw[i] - max inside the engine and, when d_sum != NULL, writes
 *    THREE values there: shard total, sum v, sum v^2 (what the ranks all-gather);
 *  - slam_ancestors_from_scan_dev and slam_offspring_from_scan_sharded_dev (whose d_shard_totals then holds such
 *    triples, [world][3]) apply the gate on the device: a frame that keeps its population gets ancestor[j] = j
 *    (first[i] = global index of i), so everything downstream — fused gathers, the exchange plan — works unchanged
 *    and nothing moves;
 *  - slam_logweight_dev / slam_logweight_ekf_dev add the carried weight of the previous frame when that frame did
 *    not resample (a device-side flag; the first frame after slam_resample_gate_set carries nothing);
 *  - slam_resample_happened_host tells the host whether the last gated resample stage did resample (it waits for a
 *    flag in mapped memory — no copy, no stream synchronisation; without a gate the answer is always 1), so that it
 *    can run the next EKF in place (map_in == map_out, no gather) instead of out of place. */
int slam_resample_gate_set(slam_engine *e, float ess_frac);
int slam_resample_happened_host(slam_engine *e, int *resampled);
/* What the last resample stage of a population with maps reported, for looking at: about how many distinct ancestors it
 * left, and the population that count belongs to (-1: nothing reported yet).  It steers the engine's choice between update
 * forms, never a result; read without any synchronisation, so it may be a frame or two old. */
int slam_resample_heads_host(slam_engine *e, int32_t *heads, int32_t *n);

/* A12: systematic resampling on the exact integer CDF.
 *  step 1 (per shard): d_cdf[i] = inclusive prefix sum of wq within the shard.
 *  step 2 (per shard): d_first[i] = number of comb teeth below the start of particle i's CDF
 *          interval = index of the first output slot it fills; needs the shard's base offset
 *          (sum of wq of all earlier shards; NULL = 0) and the grand total, both read from DEVICE
 *          memory so that the frame loop never synchronises with the host; the comb offset
 *          u = slam_comb_offset(seed, frame, total) is computed inside the kernel.
 *  step 3 (per output slot j of any shard): ancestor[j] = last global i with first[i] <= j, by
 *          binary search in the concatenated `first` array of all shards. */
int slam_prefix_sum_dev(slam_engine *e, const uint64_t *d_wq, int n, uint64_t *d_cdf);
int slam_offspring_offsets_dev(slam_engine *e, const uint64_t *d_cdf, int n, const uint64_t *d_base,
                               const uint64_t *d_total, uint64_t seed, uint32_t frame, int64_t n_total,
                               int32_t *d_first);
int slam_ancestors_dev(slam_engine *e, const int32_t *d_first_all, int64_t n_total, int64_t slot0, int nslots,
                       int32_t *d_anc);
/* Single GPU, frame-loop form: the ancestor of every one of the n slots straight from the scan left by
 * slam_quantise_scan_dev(n) — the same result as slam_offspring_from_scan_dev followed by
 * slam_ancestors_dev, in one launch and without the intermediate `first` array. */
int slam_ancestors_from_scan_dev(slam_engine *e, int n, uint64_t seed, uint32_t frame, int32_t *d_anc);
/* The comb offset of a frame: uniform integer in [0,total) from Philox4x32-10 keyed by seed,
 * counter (0,0,frame,1).  Pure host function (every rank computes the same value). */
uint64_t slam_comb_offset(uint64_t seed, uint32_t frame, uint64_t total);

/* Several GPUs (one engine per rank; n_total = world * n_local particles; world <= 16).  After the `first`
 * arrays of all ranks were all-gathered into d_first_all:
 *  - slam_ancestors_sharded_dev: the gather index of this rank's n_local slots — a local particle index when
 *    the ancestor is local, else n_local + its row in the staging tail behind the local particles.  A remote
 *    ancestor is received ONCE, however many of this rank's slots descend from it: the tail holds, in rank
 *    order and inside a rank in particle order, the distinct remote ancestors of this rank's slots.  Also writes
 *    the exchange plan of the frame to d_plan (SLAM_PLAN_WORDS(world) int32 words, device memory):
 *      [0] bit 0: some rank exchanges something this frame; bit 1: some rank's staging area (see
 *          slam_exchange_set_capacity) might not hold what it would receive — both the same on every rank,
 *      [1 .. world] send_cnt[q]: rows this rank sends to rank q,  [1+world .. 2*world] recv_cnt[q],
 *      [1+2*world .. 3*world] internal to the pack step.
 *    Needs nothing from the host; the host reads the plan once for the all-to-all's split sizes.
 *    d_pose_idx (optional, n_local words): for every slot the index of its ancestor's pose in an all-gather of
 *    the ranks' pose blocks [x[n_local] | y[n_local] | theta[n_local]] — with it the next frame's
 *    slam_motion_score_dev can run on all-gathered poses (d_src_x = gathered, d_src_y = gathered + n_local,
 *    d_src_th = gathered + 2 n_local, d_anc = d_pose_idx) before the exchange of the map rows has happened.
 *  - slam_migrate_pack_dev: one launch packs, for every destination q, its send_cnt[q] rows as records of
 *    3 + 5*nlandmarks floats (x, y, theta, then the five map planes of nlandmarks values each) — the layout of
 *    one all-to-all send buffer.  `plan` is the host copy of d_plan; uses state left by the
 *    slam_ancestors_sharded_dev call of the same frame on this engine.
 *  - slam_migrate_unpack_dev: the received records (recv_cnt[q] from rank q, same layout) into the staging
 *    tail of the pose arrays (rows x|y|theta, leading dimension pose_ld = particle capacity, which the map
 *    must have as rows too) and of the map. */
#define SLAM_PLAN_WORDS(world) (1 + 3 * (world))
int slam_ancestors_sharded_dev(slam_engine *e, const int32_t *d_first_all, int64_t n_total, int n_local, int rank,
                               int world, int32_t *d_src, int32_t *d_plan, int32_t *d_pose_idx);
/* The plan of the last slam_ancestors_sharded_dev call on this engine, on the host: the plan kernel also writes it to
 * pinned host memory mapped into the device and releases an arrival flag; this call waits for that flag (no
 * device-to-host copy, no stream synchronisation) and copies the SLAM_PLAN_WORDS(world) words out. */
int slam_exchange_plan_host(slam_engine *e, int world, int32_t *plan);
/* Rows of staging space behind the local particles (the same on every rank; <= 0 = unlimited, the initial state).
 * With it set, every later plan carries bit 1 of plan[0] when the slots of ANY rank whose ancestor lives on another
 * rank outnumber it — an upper bound of the rows that rank receives, derived from the all-gathered offsets alone, so
 * that all ranks reach the same verdict and can refuse the frame together instead of one rank failing alone. */
int slam_exchange_set_capacity(slam_engine *e, int recv_capacity);
int slam_migrate_pack_dev(slam_engine *e, int n_local, int rank, int world, const int32_t *plan, const float *d_pose,
                          int64_t pose_ld, const float *d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                          float *d_out);
int slam_migrate_unpack_dev(slam_engine *e, const float *d_in, int world, const int32_t *recv_cnt, int n_local,
                            float *d_pose, int64_t pose_ld, float *d_map, int64_t row_stride, int plane_stride,
                            int nlandmarks);

/* Index (lowest on ties) and value of the largest element: the heaviest particle. */
int slam_argmax_dev(slam_engine *e, const float *d_values, int n, int32_t *d_index, float *d_value);

/* Mean, spread and heading length of n poses in device memory, exactly as slam_pf_spread defines them (n_total = n), without a
 * session: d_idx (optional) is a pending gather — slot i holds particle d_idx[i]; d_carry (optional) is the source of the
 * 16-bit weights, one float per SLOT: logw_i - max logw, w16_i = (uint64)(det_exp(d_carry[i]) * 2^32) >> 16 (all zero: the
 * plain form).  Synchronises; the results come back by copies.  SLAM_ERR_INVALID_ARG outside the domain of slam_pf_spread. */
int slam_pose_spread_dev(slam_engine *e, const float *d_x, const float *d_y, const float *d_theta, const int32_t *d_idx,
                         const float *d_carry, int n, float ref_theta, float pose[3], float cov[6], float *heading_r);

/* One mode of a pose population: a cluster of the cloud, as slam_pf_modes defines it.  40 bytes, no padding. */
typedef struct slam_pf_mode {
    float pose[3];    /* x, y, theta: the weighted mean of the mode's members */
    float mass;       /* its share of the population's weight, in (0, 1] */
    int32_t cell[3];  /* the centre cell: ix, iy, heading bin */
    int32_t ncells;   /* occupied cells among the 27 (9 with hbins == 1) of its neighbourhood */
    int64_t weight;   /* Wm: the sum of its members' weights (particles, where the weights are equal) */
} slam_pf_mode;

/* The modes of n poses in device memory, exactly as slam_pf_modes defines them, without a session: d_idx (optional) is a pending
 * gather — slot i holds particle d_idx[i]; d_carry (optional) is the source of the 16-bit weights, one float per SLOT, exactly as
 * slam_pose_spread_dev takes it (all weights zero, or no d_carry: w = 1).  modes receives up to max_modes entries, *n_modes how
 * many, *cells the number of distinct occupied cells, *wtotal the weight of the whole population (n where w = 1).  Three launches
 * (four words of control and the table are the engine's own, made at the first call and left zeroed by every call); the
 * population is not copied and the table never leaves the device.  Synchronises; the result comes back by one copy of 480 bytes.
 * Errors, outputs untouched: SLAM_ERR_INVALID_ARG for n <= 0, a null pointer, a cell that is not finite or <= 0, hbins other than
 * 1 or 4 .. 64, max_modes outside 1 .. 8, and for a population with a particle outside the domain; SLAM_ERR_CAPACITY for more
 * than 65 536 distinct cells (choose a larger cell). */
int slam_pose_modes_dev(slam_engine *e, const float *d_x, const float *d_y, const float *d_theta, const int32_t *d_idx,
                        const float *d_carry, int n, float ref_theta, float cell, int hbins, int max_modes, slam_pf_mode *modes,
                        int *n_modes, int *cells, int64_t *wtotal);

/* Plain gather of particle attributes through an index (used when the gather is not fused into the
 * next stage, and to pack rows for migration between GPUs). */
int slam_gather_f32_dev(slam_engine *e, const float *d_src, const int32_t *d_idx, int n, float *d_dst);
/* map rows: out row i = in row d_idx[i] (strides as in slam_ekf_update_dev) */
int slam_gather_map_dev(slam_engine *e, const float *d_map_in, float *d_map_out, int64_t in_row_stride,
                        int64_t out_row_stride, int in_plane_stride, int out_plane_stride, int nlandmarks,
                        const int32_t *d_idx, int n);

/* ------------------------------------------------------------------ particle-filter session
 * Convenience object for hosts that do not manage device memory themselves (a plain C program): it owns
 * the particle arrays, the landmark maps and the resample indices on the device and runs one whole frame
 * per call by chaining the stage entry points above on the engine's stream — motion+score, EKF (when the
 * filter has landmarks and `use_observations` is set), weights, integer-CDF resample; the resample gather
 * is fused into the next frame.  slam_pf_create: one GPU; slam_pf_create_sharded (below): one session per GPU,
 * every exchange step between the GPUs issued by the engine itself.  The current scan (slam_scan_*), grid (slam_grid_*) and observation list (slam_obs_*) of the
 * engine are the frame's inputs. */
typedef struct slam_pf slam_pf;
typedef struct {
    int32_t n_particles;
    int32_t n_landmarks;   /* 0 = localisation only (weights from the scan-match score alone) */
    float sigma[3];        /* motion noise (x, y, theta) per frame */
    float meas_var;        /* landmark observation variance */
    float score_gain;      /* logw = loglik - score_gain * score */
    uint64_t seed;
    float resample_ess_frac;   /* in (0, 1): resample only when ESS < frac * N (slam_resample_gate_set); 0 = every frame */
    int32_t map_layout;        /* slam_map_layout: how the landmark maps are kept (0 = SLAM_MAP_AUTO) */
} slam_pf_config;
/* Landmark maps: ONE ROW PER PARTICLE (a resampling frame rewrites every row in full: the fastest form when a frame
 * observes most landmarks) or COPY-ON-WRITE PAGES behind a page table per particle (a resampling frame copies table
 * entries and rewrites only the pages that hold an observed landmark: the fastest form when a frame observes few of
 * many).  Both give the same bits.  SLAM_MAP_AUTO lets the session choose and change its mind while it runs. */
typedef enum { SLAM_MAP_AUTO = 0, SLAM_MAP_ROWS = 1, SLAM_MAP_PAGES = 2, SLAM_MAP_SPLIT = 3, SLAM_MAP_SPLIT_PAGES = 4 } slam_map_layout;
/* SLAM_MAP_SPLIT_PAGES (round 4): the split layout with the MEANS on copy-on-write pages of 32 landmarks x 2 planes
 * (256 bytes) and the covariances per class as in SLAM_MAP_SPLIT — what SLAM_MAP_AUTO moves a session to when its
 * frames observe few of many landmarks: a resampling frame copies table entries, rewrites only the mean pages that hold an
 * observed landmark and updates each class's covariances once.  The same bits. */
/* SLAM_MAP_SPLIT (round 4): MEANS per particle, COVARIANCES per covariance class.  The landmark update is carried out in the
 * world frame (see slam_ekf_update_dev): the posterior covariance of a landmark depends on its prior covariance, on meas_var
 * and on whether the frame observes it — never on the particle's pose or on the measurement.  Particles whose covariances are
 * equal therefore stay equal for ever (the offspring of an ancestor; a population whose maps were initialised alike), and
 * they share ONE row of covariance planes, updated once per frame, while every particle keeps its own two planes of means:
 * a resampling frame that observes every landmark reads 8 and writes 8 bytes per (particle, landmark) instead of 20 and 20.
 * Classes are found when maps come in (slam_pf_set_map_*: neighbouring particles with bit-identical covariance planes share a
 * class) and die with their last particle.  The same bits as rows and pages, on one GPU and sharded (classes are local to a
 * rank; a migrating particle becomes a class of its own where it arrives).  slam_pf_device_view gives map = NULL while a
 * session is split, like pages. */
/* SLAM_MAP_AUTO keeps a session on the SPLIT layout instead of rows (single-GPU or sharded, resampling every frame or
 * ESS-gated), and otherwise works as described here, "rows" meaning that dense layout and "pages" SLAM_MAP_SPLIT_PAGES.
 * SLAM_MAP_AUTO starts on rows and watches how many landmarks the frames observe (a count the update kernels leave in
 * mapped host memory: every frame at the start and while they speak against the current layout, every 8th frame otherwise;
 * read without waiting, except in a session's first four frames, which wait for the count of the frame before so that the
 * layout is settled by then): three counts in a row of at most
 * two sevenths of the landmarks move the maps to pages, three in a row of more than three eighths move them back (measured: split pages win
 * below 0.28-0.33 of the landmarks observed, rows and split maps above).  A move costs one
 * pass over the maps and, while it runs, half as much memory again as the steady state (one row buffer beside the pool);
 * when that is not to be had the session stays where it is.  Sessions with at most 32 landmarks stay on rows. */

int slam_pf_create(slam_engine *e, const slam_pf_config *cfg, slam_pf **out);

/* ---- several GPUs: communicators + the sharded session.
 * The reference has no multi-device code; what it does have is ONE C host program that creates
 * its accelerator handle once in main and threads it through (Submodule_2/Hadrware_acclereated.cpp:842-845, 284).
 * The sharded filter keeps that shape: a plain C host creates one engine + one communicator per GPU and then
 * drives every rank with the same slam_pf_* calls as a single GPU; the engine issues every exchange step itself
 * (RCCL over xGMI), on its own streams, with no host framework between the launches.
 *   slam_comm_unique_id      rank 0 makes the rendezvous token (ncclGetUniqueId) and hands it to the other ranks by
 *                            any means (shared memory of the host process, a file, a socket, torch.distributed ...)
 *   slam_comm_create_rccl    collective: every rank calls it with the same token (ncclCommInitRank).  One rank per
 *                            GPU; ranks may be processes or threads of one process.  world <= 16.
 *   slam_local_group_* / slam_comm_create_local
 *                            in-process transport: all ranks are threads of ONE process and exchange through
 *                            device-to-device copies and a host rendezvous.  Same results, no overlap; for hosts that
 *                            do not want RCCL and for rehearsing many ranks on few GPUs (RCCL refuses two ranks on
 *                            one device).  Every rank's calls must come from its own host thread (they block).
 * A communicator belongs to one engine and one session; destroy the session first, then the communicator. */
typedef struct slam_comm slam_comm;
typedef struct slam_local_group slam_local_group;
enum { SLAM_COMM_ID_BYTES = 128 };
int slam_comm_unique_id(uint8_t id[SLAM_COMM_ID_BYTES]);
int slam_comm_create_rccl(slam_engine *e, int rank, int world, const uint8_t id[SLAM_COMM_ID_BYTES], slam_comm **out);
int slam_local_group_create(int world, slam_local_group **out);
int slam_local_group_destroy(slam_local_group *g);
int slam_comm_create_local(slam_engine *e, slam_local_group *g, int rank, slam_comm **out);
/* Give up: after an error of its own a rank aborts its communicator so that the other ranks do not wait for it for
 * ever (ncclCommAbort / the in-process group is marked broken); every later call on it — and, once they notice, on the
 * peers' communicators — returns SLAM_ERR_COMM.  slam_pf_step does this itself when a frame of a sharded session fails
 * on this rank alone.  Host-side waits of a sharded session poll for such failures (ncclCommGetAsyncError) and give
 * up after SLAM_COMM_TIMEOUT_S seconds (environment, default 120). */
int slam_comm_abort(slam_comm *c);
int slam_comm_rank(const slam_comm *c);
int slam_comm_world(const slam_comm *c);
int slam_comm_destroy(slam_comm *c);

/* The sharded session: cfg->n_particles is THIS rank's share (the same on every rank); the population is
 * world x n_particles, particle ids are global (rank * n_particles + local index), and every result is
 * bit-identical to the same population on one GPU.  recv_capacity = rows of staging space for map rows / poses
 * that arrive from other ranks (<= 0: n_particles, which can never overflow; smaller values save memory and make
 * slam_pf_step fail with SLAM_ERR_CAPACITY — on every rank alike — in a frame whose exchange might not fit).
 * Per frame the engine issues, on its own stream and in program order with the kernels around them (no second stream,
 * no event hand-overs): all-reduce MAX of the weight normaliser, all-gather of the shard totals, all-gather of the
 * offspring offsets ("surviving indices"), an all-gather of the new poses (12 B per particle, so that the next frame's
 * motion + score launch need not wait for the exchange), and ONE grouped send/recv carrying the map rows of ancestors
 * that live on another rank (each row once per destination rank).  Every slam_pf_* call on a sharded session is
 * collective. */
int slam_pf_create_sharded(slam_engine *e, const slam_pf_config *cfg, slam_comm *comm, int recv_capacity,
                           slam_pf **out);
int slam_pf_destroy(slam_pf *pf);
/* all particles at `pose`; maps (if any) marked "not seen yet" */
int slam_pf_reset(slam_pf *pf, const float pose[3]);
int slam_pf_set_poses_host(slam_pf *pf, const float *x, const float *y, const float *theta);
int slam_pf_set_map_host(slam_pf *pf, const float *rows /* [n_particles][5][n_landmarks] */);
/* the same from device memory: rows [n_particles][5 planes][plane_stride] floats, row_stride floats apart; asynchronous */
int slam_pf_set_map_dev(slam_pf *pf, const float *d_rows, int64_t row_stride, int plane_stride);
/* Paged maps (SLAM_MAP_PAGES): every particle's landmarks sit behind a page table — pages of 32 landmarks (640 bytes),
 * shared between the offspring of an ancestor until one of them is written: a resample copies 4 bytes per 32 landmarks,
 * and a frame's update rewrites only the pages that hold an observed landmark.  For frames that observe few of many
 * landmarks (a row per particle rewrites every row on every resampling frame); results are bit-identical to a
 * row-per-particle session.  While a session is on pages it has no rows to look at: slam_pf_device_view gives map = NULL,
 * maps go in and out through slam_pf_set_map_* / slam_pf_get_map_host / slam_pf_get_map_rows_host.  Sharded sessions work
 * the same way (a migrating particle travels with all its pages, as a row does).
 * slam_pf_paged_set(e, 1): sessions created on this engine from now on with map_layout = SLAM_MAP_AUTO are kept on pages
 * (as if created with SLAM_MAP_PAGES); 0 restores AUTO's own choice.  slam_pf_is_paged: the layout right now. */
int slam_pf_paged_set(slam_engine *e, int on);
int slam_pf_is_paged(const slam_pf *pf);
/* the layout right now: SLAM_MAP_ROWS, SLAM_MAP_PAGES, SLAM_MAP_SPLIT or SLAM_MAP_SPLIT_PAGES */
int slam_pf_layout(const slam_pf *pf);
/* one frame against grid `slot`; asynchronous */
int slam_pf_step(slam_pf *pf, int slot, const float dp[3], int use_observations);
/* Scan-match refinement inside the session: with sweeps in 1..16 the first launch of every frame is motion + refine
 * (slam_motion_refine_dev) instead of motion + score, on every layout, gated or not, sharded or not; the landmark update is a
 * launch of its own that reads the refined poses, and slam_pf_view.score / count, the weights, slam_pf_best and slam_pf_mean
 * all see the refined poses and their scores.  sweeps = 0 (the initial state; the steps are then ignored) switches it off.
 * Sharded: every rank must make the same call. */
int slam_pf_refine_set(slam_pf *pf, float step_xy, float step_theta, int sweeps);
/* A full 2x2 measurement covariance for the session's landmark update (slam_ekf_update_aniso_dev; meas_cov = {qxx, qxy,
 * qyy}, the same conditions).  Legal between frames; sharded: every rank must make the same call.  Only a session created
 * with map_layout = SLAM_MAP_ROWS and n_landmarks > 0 stores a covariance per particle: any other session returns
 * SLAM_ERR_INVALID_ARG (slam_last_error says so) and goes on as before.  From then on every frame's update is that stage as a
 * launch of its own — out of place, in place on the frames a gated session kept its population, through the staging tail
 * when sharded — and no frame goes out as a fused front launch.  meas_cov = {cfg.meas_var, 0, cfg.meas_var} switches back:
 * the session then runs exactly what it ran before the first call. */
int slam_pf_meas_cov_set(slam_pf *pf, const float meas_cov[3]);
/* Data association inside the session (slam_associate_dev + slam_ekf_update_assoc_dev with cfg.meas_var).  After a call with
 * gate > 0 a frame with use_observations ignores the observation table and reads the engine's DETECTIONS
 * (slam_detections_upload_host / _set_dev; none handed over: SLAM_ERR_NOT_READY): it runs associate and then update, two
 * launches that read the refined poses when refinement is on and work in place on the frames a gated session kept; no frame
 * goes out as a fused front launch.  Only a single-GPU session created with map_layout = SLAM_MAP_ROWS and n_landmarks > 0
 * accepts the switch: any other layout, a sharded session, and a session with a non-isotropic slam_pf_meas_cov_set in force
 * return SLAM_ERR_INVALID_ARG (slam_last_error says why) and go on as before; setting a 2x2 covariance while association is
 * on is refused likewise.  gate == 0 (new_gate and create are then ignored) returns the session to exactly what it ran before.
 * slam_pf_assoc_device_view: the table ([n_particles][*assoc_stride] bytes) and stats ([n_particles][3]) of the last such
 * frame, indexed like slam_pf_view.score (BEFORE the pending gather); SLAM_ERR_NOT_READY until association was switched on.
 * The noise form given anew: a call with gate > 0 — this one, slam_pf_assoc_cov_set or slam_pf_assoc_detcov_set, which both go
 * through it — on a session that already associates changes the noise form and the gates and NOTHING else: pruning and its
 * evidence bytes, line of sight, field of view, merging and the detector (slam_pf_prune_set, slam_pf_prune_sight_set,
 * slam_pf_prune_fov_set, slam_pf_merge_set, slam_pf_detect_*_set) stay as they were.  Only gate == 0 clears them, all of them;
 * switched on again afterwards the session runs as a fresh one would from its poses and maps (slam_pf_prune_set makes the
 * evidence from the maps again).  tests/_pipeline_spec.py states this, and tests/test_gpu_pipeline_session.py holds the session to it. */
int slam_pf_assoc_set(slam_pf *pf, float gate, float new_gate, int create);
int slam_pf_assoc_device_view(slam_pf *pf, const uint8_t **assoc, int32_t *assoc_stride, const int32_t **stats);
/* Data association under a 2x2 measurement covariance inside the session: ONE switch that sets covariance and gates together
 * (slam_associate_aniso_dev + slam_ekf_update_assoc_aniso_dev with meas_cov in every observing frame).  The conditions of
 * slam_pf_assoc_set (single-GPU rows, n_landmarks > 0 and <= SLAM_MAX_OBS, the gates' rules; gate == 0 is refused here: off is
 * slam_pf_assoc_set(0, ..)) and those of slam_pf_meas_cov_set on meas_cov; refused, like slam_pf_assoc_set, while a non-isotropic
 * slam_pf_meas_cov_set is in force — there is one way in, and the session never holds two matrices that could disagree.  It
 * allocates the table as slam_pf_assoc_set does, and everything that accepts an associating session accepts this one
 * (slam_pf_prune_set, slam_pf_detect_set, slam_pf_assoc_device_view, refinement, the resample gate's in-place frames); no frame
 * goes out as a fused front launch.  meas_cov = {cfg.meas_var, 0, cfg.meas_var} is exactly slam_pf_assoc_set(gate, new_gate,
 * create): the isotropic kernels, the same bits.  While it is on, slam_pf_meas_cov_set(non-isotropic) stays refused (association
 * is on), slam_pf_assoc_set(gate > 0, ..) returns the session to isotropic association and slam_pf_assoc_set(0, ..) switches
 * association off.  Not implemented: the split, paged, AUTO and sharded forms, an evidence stage fused into the update, more than
 * SLAM_MAX_DETECTIONS detections. */
int slam_pf_assoc_cov_set(slam_pf *pf, const float meas_cov[3], float gate, float new_gate, int create);
/* ... under the covariance EACH DETECTION carries (slam_detections_cov_upload_host / _set_dev): every observing frame runs
 * slam_associate_detcov_dev + slam_ekf_update_assoc_detcov_dev.  The conditions and refusals of slam_pf_assoc_set (rows,
 * n_landmarks > 0, one GPU, no slam_pf_meas_cov_set in force; gate = 0 is refused here: slam_pf_assoc_set(0, ..) switches off); a
 * refused call leaves the session as it was.  slam_pf_assoc_set(gate > 0) afterwards returns to isotropic association,
 * slam_pf_assoc_cov_set to one Q.  Pruning, refinement and the resample gate (the in-place update on kept frames included) are
 * accepted as on any associating session; no frame fuses its front.  An observing frame whose detections carry no covariance —
 * no detector and none attached since the last hand-over, or a detector without a noise model (slam_pf_detect_set /
 * slam_pf_detect_fit_set; slam_pf_detect_noise_set gives it one) — returns SLAM_ERR_NOT_READY before its first launch: the session is unchanged and the next good frame runs as if the
 * bad one was never asked for. */
int slam_pf_assoc_detcov_set(slam_pf *pf, float gate, float new_gate, int create);
/* Pruning of clutter landmarks inside the session (slam_landmark_evidence_dev behind every associating update).  Accepted only
 * while association is on — so never off single-GPU rows: otherwise SLAM_ERR_INVALID_ARG (slam_last_error says why) and the
 * session goes on as before; likewise for hit, miss or cmax outside 1 .. 255 or a view_range that is not finite and > 0.
 * hit == 0 switches pruning off (the other arguments are then ignored), and so does slam_pf_assoc_set(gate = 0); with pruning
 * off the session runs exactly what it ran before the first call.  Switching on allocates (once) two evidence buffers
 * [n_particles][ev_stride] and the stats, and initialises the evidence of the CURRENT maps with value = cmax: a map that is
 * there is trusted.  The same initialisation runs whenever the maps are replaced wholesale while pruning is on
 * (slam_pf_set_map_host / _dev, slam_pf_reset).  Frames: the stage runs behind the associating update on the row it wrote —
 * through the frame's gather into the other evidence buffer, or in place on the frames a gated session kept; a frame without
 * observations gathers the evidence as it gathers the maps.
 * slam_pf_evidence_device_view: the current evidence ([n_particles][*ev_stride] bytes, indexed like slam_pf_view.map: BEFORE the
 * pending gather) and the stats ([n_particles][2], indexed like slam_pf_view.score) of the last frame that ran the stage.
 * slam_pf_get_evidence_host: [n_particles][n_landmarks] with the pending gather applied, like slam_pf_get_map_host;
 * synchronises.  Both: SLAM_ERR_NOT_READY until pruning was switched on. */
int slam_pf_prune_set(slam_pf *pf, int hit, int miss, int cmax, float view_range);   /* hit == 0: off */
int slam_pf_evidence_device_view(slam_pf *pf, const uint8_t **ev, int32_t *ev_stride, const int32_t **stats);
int slam_pf_get_evidence_host(slam_pf *pf, uint8_t *ev /* [n][nlandmarks] */);       /* pending gather applied, like slam_pf_get_map_host */
/* Line of sight inside the session.  Accepted where slam_pf_prune_set is (only while association is on; otherwise, or for bins
 * that are no power of two in 32 .. 1024 or a margin that is not finite and > 0: SLAM_ERR_INVALID_ARG, and the session goes on as
 * before); it is IN FORCE only while pruning is on.  bins == 0 switches it off, and so does slam_pf_assoc_set(gate = 0); with it
 * off the session runs exactly what it ran before the first call, and slam_sight_counts does not move.  In force, the evidence
 * stage of an observing frame is one slam_sight_table_dev(bins) over the engine's current scan (the scan the frame scores and
 * the detector reads) and then slam_landmark_evidence_sight_dev in the place of slam_landmark_evidence_dev: the same evidence
 * buffers, the same stats.  Switching on allocates (once) the spared counts; no frame allocates.
 * slam_pf_sight_device_view: the engine's table (1024 floats, the first *bins in use), the bins in force (0: off) and the spared
 * counts ([n_particles], indexed like slam_pf_view.score) of the last frame that ran the stage.  SLAM_ERR_NOT_READY until line
 * of sight was switched on. */
int slam_pf_prune_sight_set(slam_pf *pf, int bins /* 0: off */, float margin);
int slam_pf_sight_device_view(slam_pf *pf, const float **table, int32_t *bins, const int32_t **spared);
/* The field of view inside the session.  Accepted where slam_pf_prune_sight_set is (only while association is on); IN FORCE only
 * while pruning is on; on == 0 switches it off, and so does slam_pf_assoc_set(gate = 0); with it off the session runs exactly what
 * it ran before the first call, launch for launch, and slam_fov_counts does not move.  The arc is [angle_min + edge, angle_max -
 * edge] in radians of the sensor frame (float32 sums): lo = slam_fov_bound(angle_min + edge), hi = slam_fov_bound(angle_max -
 * edge); edge >= 0 narrows the view at both ends — it covers the strip in which the detector (wrap = 0) drops the segments that
 * touch the edge of the view.  SLAM_ERR_INVALID_ARG (and the session goes on as before) for a value that is not finite, edge < 0,
 * angle_min < -pi or angle_max > pi (float32 pi), or angle_min + edge >= angle_max - edge.  In force, the evidence stage of an
 * observing frame is slam_landmark_evidence_fov_dev in the place of slam_landmark_evidence_dev (use_sight = 0) or, with line of
 * sight on, behind its slam_sight_table_dev in the place of slam_landmark_evidence_sight_dev (use_sight = 1): the same evidence
 * buffers, the same stats.  Switching on allocates (once) the outside counts; no frame allocates.
 * slam_pf_fov_device_view: the bounds in force (0, 4 while it is off: everything in view) and the outside counts ([n_particles],
 * indexed like slam_pf_view.score) of the last frame that ran the stage.  SLAM_ERR_NOT_READY until it was switched on. */
int slam_pf_prune_fov_set(slam_pf *pf, int on, float angle_min, float angle_max, float edge);
int slam_pf_fov_device_view(slam_pf *pf, float bounds[2], const int32_t **outside);
/* Merging inside the session (slam_landmark_merge_dev).  merge_gate == 0 switches it off, and so does slam_pf_assoc_set(gate =
 * 0); with it off the session runs exactly what it ran before the first call, launch for launch, and slam_merge_count does not
 * move.  Accepted only while association is on — under any of its three noise forms (slam_pf_assoc_set, slam_pf_assoc_cov_set,
 * slam_pf_assoc_detcov_set): the rule reads only the landmarks' own covariances — otherwise SLAM_ERR_INVALID_ARG (slam_last_error
 * says why), as slam_pf_prune_set refuses: split, paged, AUTO and sharded sessions never get there.  SLAM_ERR_INVALID_ARG too for a
 * gate that is not finite or < 0.  A refused call leaves the session unchanged.  In force, every frame with use_observations runs
 * the stage behind its update and its evidence stage, on the rows that frame wrote (the other map buffer, or in place on a frame
 * a gated session kept) and — while pruning is on — on the evidence buffer it wrote with the pruning's cmax; with pruning off,
 * without evidence.  Switching on allocates (once) the stats; no frame allocates.
 * slam_pf_merge_device_view: the stats ([n_particles][3] = merged, refused, seen after; indexed like slam_pf_view.score) of the
 * last frame that ran the stage.  SLAM_ERR_NOT_READY until merging was switched on. */
int slam_pf_merge_set(slam_pf *pf, float merge_gate /* 0: off */);
int slam_pf_merge_device_view(slam_pf *pf, const int32_t **stats);
/* The weight of the unexplained inside the session (slam_assoc_weight_dev).  on == 0 switches it off, and so does
 * slam_pf_assoc_set(gate = 0); a noise form given anew leaves it as it was.  With it off the session runs exactly what it ran
 * before the first call, launch for launch, and slam_assoc_weight_count does not move.  Accepted where slam_pf_merge_set is — only
 * while association is on, under any of its three noise forms — otherwise SLAM_ERR_INVALID_ARG (slam_last_error says why): split,
 * paged, AUTO and sharded sessions never get there.  SLAM_ERR_INVALID_ARG too for a constant that is not finite or > 0.  A refused
 * call leaves the session unchanged.  In force, every frame with use_observations runs its evidence stage (while pruning is on) in
 * the _missed form and the stage behind its update, evidence stage and merge, in front of the weights, on the engine's
 * log-likelihood buffer; a frame without a hand-over runs neither.  Merging runs behind the evidence stage and does not change the
 * counts.  (0, 0, 0) is a valid "on": the weights are bit for bit those of "off".  A non-zero log_miss while pruning is off is
 * accepted and inert: nothing scores a miss.  Calling it again changes the constants from the next frame on.  Switching on
 * allocates (once) the two buffers below; no frame allocates.
 * slam_pf_assoc_weight_device_view: of the last frame that ran the stage, indexed like slam_pf_view.score — missed int32
 * [n_particles] (NULL while pruning is off) and terms float32 [n_particles], the t that was added.  SLAM_ERR_NOT_READY until the
 * switch was on once. */
int slam_pf_assoc_weight_set(slam_pf *pf, float log_new, float log_clutter, float log_miss, int on);
int slam_pf_assoc_weight_device_view(slam_pf *pf, const int32_t **missed, const float **terms);
/* The detector inside the session (slam_detect_scan_dev with these parameters; NULL: off).  Accepted only while association is on
 * — otherwise SLAM_ERR_INVALID_ARG (slam_last_error says why) and the session goes on as before; likewise for parameters that
 * slam_detect_scan_dev refuses.  slam_pf_assoc_set(gate = 0) switches it off too.  With it on, every frame with use_observations
 * makes its detections from the engine's current scan — the launch goes out in front of the frame's first launch, so its count
 * has long arrived when the association asks for it — and then runs associate -> update (-> evidence) on them; whatever
 * detections were handed over are replaced.  With it off the session runs exactly what it ran before the first call. */
int slam_pf_detect_set(slam_pf *pf, const slam_detect_params *params /* NULL: off */);
/* ... with the fit (slam_detect_scan_fit_dev): accepted and refused exactly where slam_pf_detect_set is, and for a fit that
 * slam_detect_scan_fit_dev refuses.  params == NULL: the detector off; fit == NULL: slam_pf_detect_set(params).
 * slam_pf_detect_set and slam_pf_assoc_set(gate = 0) clear the fit.  The frame's launches and their order are the same. */
int slam_pf_detect_fit_set(slam_pf *pf, const slam_detect_params *params /* NULL: off */, const slam_detect_fit *fit /* NULL: the centroid */);
/* ... with the noise model (slam_detect_scan_noise_dev): accepted and refused exactly where slam_pf_detect_fit_set is — in any
 * associating mode; the two older modes ignore the covariances — and for a model that slam_detect_scan_noise_dev refuses.
 * noise == NULL: slam_pf_detect_fit_set(params, fit).  Under slam_pf_assoc_detcov_set this is the detector whose frames run. */
int slam_pf_detect_noise_set(slam_pf *pf, const slam_detect_params *params /* NULL: off */, const slam_detect_fit *fit /* NULL: the centroid */,
                             const slam_detect_noise *noise /* NULL: no model */);
/* Localisation in a known map inside the session (slam_known_map_prepare_dev at the switch, slam_localise_dev per frame; the
 * session's frame loop: tests/_localise_spec.py frame_loop).  rows: host float32 [5][nlandmarks], planes mx, my, P_xx, P_xy, P_yy,
 * P_xx < 0: the slot holds no landmark; the noise is the session's meas_var * I.  rows == NULL switches the mode off (and the
 * detector with it): the session then runs exactly what it ran before the first call.  Accepted on a session created with
 * n_landmarks == 0 on one GPU, whatever its map_layout (it has no maps).  SLAM_ERR_INVALID_ARG (slam_last_error says why), the
 * session left as it was: a session with n_landmarks > 0; a sharded session; nlandmarks < 1 or > SLAM_MAX_OBS; a gate that is not
 * finite and > 0; a log_clutter that is positive, NaN or infinite; a map value that is not finite; a landmark with P_xx + meas_var
 * <= 0, P_yy + meas_var <= 0 or det (P + meas_var I) <= 0.  Everything is allocated at the switch, no frame allocates; calling it
 * again replaces map and constants from the next frame on.
 * While it is on, slam_pf_step(.., use_observations = 1) runs front launch (a refining session: motion + refine, and the REFINED
 * poses go to the stage), the stage on the engine's current detections, slam_assoc_weight_dev with log_new = log_miss = 0 and no
 * misses (left out when log_clutter == 0), slam_logweight_ekf_dev, scan, resample; a frame with use_observations = 0 is the
 * frame of a session without the mode: plain weights.  slam_pf_detect_set / slam_pf_detect_fit_set are accepted while it is on
 * (the detector's launch goes out in front of the frame's first launch); slam_pf_detect_noise_set with a model is refused: the
 * noise is meas_var * I only (slam_pf_known_map_detcov_set is the form that takes it).  Out of scope: sharded sessions,
 * pruning, merging.
 * slam_pf_known_map_detcov_set (the frame loop: tests/_localise_detcov_spec.py frame_loop) is the same switch for the second
 * form of the stage: every observing frame runs slam_localise_detcov_dev on the map as it was given, under the covariances its
 * detections carry; meas_var is not read.  Accepted and refused where slam_pf_known_map_set is, except that the landmarks'
 * covariances are checked on their own: P_xx >= 0 (else the slot holds no landmark), P_yy >= 0 and det P >= 0.  rows == NULL
 * switches the mode off; either switch replaces the other, map and constants, from the next frame on (slam_pf_known_map_set
 * drops the detector's noise model, which it does not take; the detector itself stays on).  While it is on
 * slam_pf_detect_noise_set with a model is accepted, and the frame is: the detector's launch (in its noise form), the front
 * launch, slam_localise_detcov_dev, slam_assoc_weight_dev (left out at log_clutter == 0), slam_logweight_ekf_dev, scan, resample.
 * An observing frame whose detections will carry no covariance (none uploaded and no detector, or a detector without a model)
 * returns SLAM_ERR_NOT_READY before its first launch and leaves the session unchanged.
 * slam_pf_known_map_device_view: the prepared map ([6][nlandmarks rounded up to 32]; NULL while the mode is off and under
 * slam_pf_known_map_detcov_set, which prepares none; nlandmarks 0 while the mode is off) and the
 * stats ([n_particles][3] = matched, 0, dropped; indexed like slam_pf_view.score) of the last frame that ran the stage; any of the
 * three pointers may be NULL.  SLAM_ERR_NOT_READY until a map was accepted once. */
int slam_pf_known_map_set(slam_pf *pf, const float *rows /* host [5][nlandmarks]; NULL: off */, int nlandmarks,
                          float gate, float log_clutter);
int slam_pf_known_map_detcov_set(slam_pf *pf, const float *rows /* host [5][nlandmarks]; NULL: off */, int nlandmarks,
                                 float gate, float log_clutter);
int slam_pf_known_map_device_view(slam_pf *pf, const float **prepared, int32_t *nlandmarks, const int32_t **stats);
/* The landmarks in view that no detection matched, inside the session (the frame loop: tests/_localise_miss_spec.py frame_loop).
 * Accepted only while a known map of either form is set (else SLAM_ERR_INVALID_ARG); view_range == 0 switches it off; switching
 * the known map off switches it off too, replacing the map keeps it.  log_miss finite and <= 0 (0 with a view is valid: the counts
 * are made and nothing is added); view_range finite and > 0; fov_on, angle_min, angle_max, edge as slam_pf_prune_fov_set (fov_on
 * == 0: the whole circle, the three are not read); sight_bins (0: no line of sight) and margin as slam_pf_prune_sight_set.  A
 * refused call leaves the session as it was.  With it off a frame runs exactly the launches it ran before the first call.  With
 * it on an observing frame runs, behind the front launch: slam_sight_table_dev (only with line of sight), slam_localise_miss_dev
 * or slam_localise_detcov_miss_dev in the place of the stage, slam_assoc_weight_dev(stats, missed, 0, log_clutter, log_miss) (left
 * out only when both constants are 0), slam_logweight_ekf_dev, scan, resample.  Still one GPU, n_landmarks == 0.
 * slam_pf_known_map_miss_device_view: missed, spared, outside, int32 [n_particles] each (indexed like slam_pf_view.score), of the
 * last frame that ran the miss form; any pointer may be NULL.  SLAM_ERR_NOT_READY until the misses were switched on once. */
int slam_pf_known_map_miss_set(slam_pf *pf, float log_miss, float view_range,
                               int fov_on, float angle_min, float angle_max, float edge,   /* as slam_pf_prune_fov_set */
                               int sight_bins /* 0: off */, float margin);                 /* as slam_pf_prune_sight_set */
int slam_pf_known_map_miss_device_view(slam_pf *pf, const int32_t **missed, const int32_t **spared, const int32_t **outside);
/* Reseeding inside the session (slam_pose_reseed_dev; the frame loop: tests/_reseed_spec.py frame_loop): what to do about a cloud
 * that settled on a wrong pose, was moved while it was not looking, or never knew where it started.  Called BETWEEN frames on a
 * session whose known-map mode is on, in either noise form; it reads the map as it was given.  One launch applies the pending
 * resample and the proposals: it reads the current poses through the pending gather and writes the other pose buffer, which
 * becomes the current one; no gather is pending afterwards, and a gated session drops the weights it would have carried (as
 * slam_pf_set_poses_host does).  The detections are the engine's current ones — those of the frame just run, unless the host handed
 * over others since; first_id = 0, the seed is the session's, and the Philox frame word is the session's frame counter (the number
 * of the NEXT frame): two calls with no slam_pf_step between them draw the same slots, landmarks, detections and headings.
 * counts = {replaced, chosen but not replaced}; the call waits for the two words in mapped host memory and for nothing else (a
 * gated session: the stream, where it drops the weights).  K == 0: SLAM_OK, counts 0, the session is as it was.
 * After a successful reseed the last frame's log-weights no longer belong to the poses: slam_pf_best returns SLAM_ERR_NOT_READY
 * (slam_last_error says why) until the next slam_pf_step; slam_pf_mean, slam_pf_spread and slam_pf_get_poses_host see the reseeded
 * population with equal weights, as after slam_pf_set_poses_host.  A session that never calls it runs exactly what it ran before.
 * SLAM_ERR_NOT_READY, the reason in slam_last_error and the session as it was: the mode is off; the session is sharded; it has
 * n_landmarks > 0; no detections were handed over.  SLAM_ERR_INVALID_ARG: a null pointer, a fraction outside (0, 1]. */
int slam_pf_known_map_reseed(slam_pf *pf, float fraction, int32_t counts[2]);
/* The same with proposals from detection pairs (slam_pose_reseed_pairs_dev; the frame loop: tests/_reseed_pair_spec.py frame_loop):
 * every state rule of slam_pf_known_map_reseed holds — between frames, known-map mode on in either noise form, first_id = 0, the
 * session's seed and frame counter (two calls with no step between them draw the same), the pending resample rides along, a gated
 * session drops its carried weights, slam_pf_best is refused until the next slam_pf_step.  counts = {replaced, j1 empty, too close,
 * no partner}, through four words of the mapped result block behind its sequence number.  Fewer than two detections: SLAM_OK,
 * counts 0, the session is as it was.  SLAM_ERR_NOT_READY as there; SLAM_ERR_INVALID_ARG: a null pointer, a fraction outside (0, 1],
 * !(tol >= 0), !(min_sep > tol), a non-finite value of either, a known map of fewer than two landmark slots. */
int slam_pf_known_map_reseed_pairs(slam_pf *pf, float fraction, float tol, float min_sep, int32_t counts[4]);
/* heaviest particle of the last frame (lowest index on ties; a NaN log-weight never wins; nothing but -inf and NaN:
 * particle 0 with log-weight -inf): its pose, log-weight and index; synchronises.  SLAM_ERR_NOT_READY between a successful
 * slam_pf_known_map_reseed (or _reseed_pairs) and the next slam_pf_step.
 * Sharded: the heaviest of the whole population (the same answer on every rank), `index` is its global id. */
int slam_pf_best(slam_pf *pf, float pose[3], float *logw, int32_t *index);
/* Posterior mean of the current population: x and y are averaged, the heading is averaged on the circle around
 * `ref_theta` (theta = ref + atan2(sum sin(theta_i - ref), sum cos(theta_i - ref)), so a population straddling +-pi does
 * not average to nonsense and theta stays unwrapped — the reference never normalises angles; pass the
 * predicted heading).  The sums are exact fixed-point integer sums made on the device, X_i = trunc(x_i * 2^32) and Y_i
 * likewise, S_i / C_i = trunc(sin / cos(theta_i - ref) * 2^30) (the cast of C: towards zero), so the result is
 * bit-identical for any workgroup count and any number of GPUs.
 *   Frames that resampled, sessions without a gate and sessions before their first step (equal weights): the plain mean,
 *     x = float(double(sum X) / 2^32 / n_total), theta = float(ref + atan2(double(sum S), double(sum C)));
 *   one launch, the four sums land in mapped host memory (no copy of the population, no stream synchronisation).
 *   Domain: the sums are 64-bit, |sum X| <= n_total * max|x| * 2^32 must stay below 2^63: n_total * max|x| < 2^31 metres
 *   (256 m at 2^23 particles; |S|, |C| <= 2^30 never get there with n_total < 2^31).
 *   Frames the resample gate kept (cfg.resample_ess_frac in (0, 1), the last frame did not resample): the particles carry
 *   unequal weights, and particle i counts with the 16-bit weight the gate's own sums are made of,
 *     w16_i = (uint64)(det_exp(logw_i - max logw) * 2^32) >> 16,    D = sum w16 (the gate's S),
 *     Qx = trunc(sum w16_i X_i / D) (Qy, Qs, Qc alike),  x = float(double(Qx) / 2^32),  theta = float(ref + atan2(Qs, Qc)).
 *   The device sums every product as two limbs, w16 * (V >> 21) and w16 * (V & 0x1fffff), the host joins them in 128 bits.
 *   Domain: w16 <= 2^16 and |V >> 21| <= 2^21 for |x|, |y| <= 1024 m, so a limb product is at most 2^37 and the sum of
 *   n_total <= 2^23 of them at most 2^60 < 2^63; the call waits for the gate's verdict and for the nine sums (a copy).
 *   set_poses / reset discard the carried weights: the mean after them is the plain one again.
 * Sharded: collective, the same answer on every rank. */
int slam_pf_mean(slam_pf *pf, float ref_theta, float pose[3]);
/* The mean together with the spread of the population about it: has the cloud settled?  `pose` is exactly what
 * slam_pf_mean(pf, ref_theta, pose) returns, bit for bit — the plain mean where that is plain, the weighted one on a frame the
 * resample gate kept; call it (mx, my, mt).  A second launch then forms, per particle (behind the pending gather),
 *     dx = x_i - mx,  dy = y_i - my  (one binary32 subtraction each),  s_i = sin_det(theta_i - mt)  (one binary32 subtraction,
 *     then the specified polynomial of the mean),  DX = trunc(dx * 2^20), DY and SS likewise (the cast of C: towards zero),
 * and the six exact integer sums of w_i * A_i * B_i for (A, B) = (DX,DX) (DX,DY) (DY,DY) (DX,SS) (DY,SS) (SS,SS) with D = sum w_i:
 * w_i = 1 and D = n_total where the mean is plain, w_i = w16_i and D = the gate's S where it is weighted.  Then
 *     cov[k] = float(double(trunc(sum_k / D)) / 2^40)    in that order:  xx, xy, yy, xs, ys, ss
 * — the 3 x 3 covariance over (x, y, sin(theta - mt)) in its population (biased) form about the mean the call returns.  The sine
 * of a heading difference is the difference itself for a settled cloud and saturates for a spread one, so the call also returns
 *     *heading_r = float(hypot(double(Qs), double(Qc)) / 2^30),
 * the length of the mean heading vector from the mean's own sums (Qs, Qc as above; where the mean is plain
 * Qs = trunc(sum S / n_total), Qc likewise): 1 = one heading, near 0 = headings all round the circle.
 * n = 1 and a population of identical poses give +0 in all six entries and heading_r = 1 up to the truncation of C.
 * A SMALL SPREAD SAYS THAT THE PARTICLES AGREE, NOT THAT THEY ARE RIGHT: a cloud that settled on a wrong pose reports the same
 * (what to do about such a cloud in a known map: slam_pf_known_map_reseed).
 *   Domain: |dx|, |dy| < 2048 m, so |DX|, |DY| < 2^31 and a product P = A * B is one 32 x 32 -> 64-bit multiply, |P| < 2^62.  The
 *   device sums w * P as three limbs, w * (P & 0x1fffff), w * ((P >> 21) & 0x1fffff) and w * (P >> 42): with w <= 2^16 a term is
 *   below 2^37 in size and n_total <= 2^23 of them below 2^60 < 2^63 in every 64-bit accumulator; the host joins the limbs in
 *   128 bits.  A delta outside the domain never gives a silently wrong number: the kernel counts such particles in a flag word
 *   and the call returns SLAM_ERR_INVALID_ARG (slam_last_error says why) without writing its outputs.  The domains of
 *   slam_pf_mean hold as well.  NaN poses are the caller's error, as for the mean: the result is then unspecified (a NaN in x or y
 *   fails the domain test; a NaN heading does not).
 *   One GPU: two launches, each delivering through mapped host memory (on kept frames the mean's nine sums come by a copy, as in
 *   slam_pf_mean); no copy of the population.  set_poses / reset discard the carried weights; before the first step the answer
 *   is the plain form.
 * Sharded: collective, supported — two exchanges (the mean must be the global one before the second launch), the integer sums
 * add over the ranks in any order, the same answer (and the same verdict on the domain) on every rank. */
int slam_pf_spread(slam_pf *pf, float ref_theta, float pose[3], float cov[6], float *heading_r);
/* The modes of the population: where mean and spread assume one hump, this call names the few heaviest clusters of the cloud, each
 * with a pose and a mass — "settled, 97 % in one mode", "two candidates at 55 / 40 %", "proposals gather at a second place".  A
 * function of the population alone (behind the pending gather), never of the schedule: a permuted population gives the same bytes.
 *   Per particle, every operation one binary32 rounding, inv = 1.0f / cell formed once on the host:
 *     u = x * inv;  fl = floorf(u);  ix = (int32)fl  (floor, not the cast);  FX = (int32)((u - fl) * 2^20);  iy, FY likewise from y;
 *     t = theta * 0.15915494f;  t = t - floorf(t);  b = min((int32)(t * (float)hbins), hbins - 1);
 *     (s, c) = sincos_det(theta - ref_theta);  S = trunc(s * 2^20), C = trunc(c * 2^20).
 *   (u - fl is exact and in [0, 1) except for u in (-2^-25, 0), where it rounds to 1.0f: FX = 2^20 in cell -1, the same place.)
 *   Domain: |u| < 2^20 in x and in y and a finite heading; a NaN anywhere is outside.  Particles outside are counted, and if there
 *   is one the call returns SLAM_ERR_INVALID_ARG without writing its outputs (slam_last_error says how many).
 *   Weights as in slam_pf_spread, word for word: w = 1 before the first step, on frames that resampled, after slam_pf_set_poses,
 *   slam_pf_reset and either reseed; the gate's 16-bit weights w16 on a frame the resample gate kept (all of them zero: w = 1).
 *   A particle of weight 0 contributes nothing and makes no cell.
 *   A cell is a distinct key (ix, iy, b) with five exact integer sums: W = sum w, sum w FX, sum w FY, sum w S, sum w C (with
 *   n_total <= 2^23 and w <= 2^16 every sum stays below 2^59: one 64-bit accumulator each).  More than 65 536 distinct cells:
 *   SLAM_ERR_CAPACITY, outputs untouched — a verdict on the set of keys, not on the order they arrived in.
 *   The score of a cell is W summed over its neighbourhood: |dix| <= 1, |diy| <= 1 and cyclic heading distance <= 1 (mod hbins) —
 *   27 cells, 9 with hbins == 1.  Rounds r = 0 .. max_modes - 1: a cell is eligible unless an earlier centre lies within
 *   |dix| <= 2, |diy| <= 2 and cyclic heading distance <= 2 of it, all three at once (so the neighbourhoods of centres are
 *   disjoint); the eligible cell of the largest score is the centre of mode r, the smallest (ix, iy, b) — signed, in that order —
 *   on ties; no eligible cell ends the list (*n_modes may be less than max_modes).
 *   The mode of a centre (ix0, iy0, b0): its members are the occupied cells of its neighbourhood; Wm = sum W;
 *     A = sum over members (W * (ix - ix0) * 2^20 + sum w FX),  Q = trunc(A / Wm),
 *     pose[0] = float((double(ix0) + double(Q) / 2^20) * double(cell)),   pose[1] likewise;
 *     pose[2] = float(double(ref_theta) + atan2(double(sum w S), double(sum w C)))  (atan2(0, 0) = 0);
 *     mass = float(double(Wm) / double(Wtotal)),  Wtotal over all cells.
 *   *cells receives the number of distinct cells.
 *   A cluster wider than three cells is reported as neighbouring modes two or more cells on: choose cell at least the size of a
 *   settled cloud.  hbins is 1 (headings ignored) or 4 .. 64; max_modes 1 .. 8; cell finite and > 0.
 *   Allowed wherever slam_pf_spread is — also between a reseed and the next step, where slam_pf_best is not.  Three launches
 *   (accumulate, score, select), the result through mapped host memory; the table (16 MB) is made by the first call, not with the
 *   session: a session that never calls this runs exactly the launches it ran before.  No policy: what to do with the answer is
 *   the application's.
 * Sharded sessions: NOT BUILT (adding cells over ranks) — SLAM_ERR_INVALID_ARG, as slam_pf_known_map_set answers them. */
int slam_pf_modes(slam_pf *pf, float ref_theta, float cell, int hbins, int max_modes, slam_pf_mode *modes, int *n_modes, int *cells);
/* rows this rank received in the exchange of the last completed frame (0 on a single GPU) */
int slam_pf_rows_received(const slam_pf *pf);
/* With cfg.resample_ess_frac in (0, 1): how many of the frames the host has looked at so far did resample (the
 * verdict of a frame is read at the start of the next one).  Without a gate: 0 (every frame resamples). */
int64_t slam_pf_frames_resampled(const slam_pf *pf);
/* how often a SLAM_MAP_AUTO session has moved its maps between rows and pages so far */
int64_t slam_pf_layout_changes(const slam_pf *pf);
/* The session's CURRENT device buffers, for hosts that fill or inspect the population on the device instead of
 * through the *_host copies (a 52 GB map does not want to pass through host memory): pose = [x | y | theta] of
 * n_particles floats each; map = one row per particle, row_stride floats apart, five planes of plane_stride floats
 * (layout of slam_ekf_update_dev); anc = the pending resample gather (slot i descends from particle anc[i] of
 * these buffers; NULL when none is pending: right after create / reset / set_*).  The pointers move with every
 * slam_pf_step; synchronise (slam_engine_sync) before touching the memory from another stream.
 * This call and the two *_device_view calls below may ISSUE A LAUNCH on the engine's stream: after a survivor-rows frame
 * (slam_survivor_rows_set) they first have every mean row of that frame written.  Ask for the view again after every
 * slam_pf_step: a view kept across a step may show rows that nobody has written yet. */
typedef struct {
    float *pose, *map;
    float *map_spare;                 /* the other map buffer: free between frames (the next EKF writes it) */
    const int32_t *anc;
    int64_t row_stride;
    int32_t plane_stride, map_rows;   /* map_rows = n_particles + staging rows (sharded) */
    /* what the last slam_pf_step left behind, indexed like `pose` (i.e. BEFORE the pending gather): the scan-match
     * score, the log-weight and — when that frame used observations, else NULL — the EKF log-likelihood of every
     * particle; NULL before the first frame */
    const float *score, *logw, *loglik;
    const int32_t *count;             /* in-bounds beams behind `score` (main.c:512-518 counts them as bestHits_size) */
} slam_pf_view;
int slam_pf_device_view(slam_pf *pf, slam_pf_view *out);
/* current particles with the pending resample gather applied; synchronises */
int slam_pf_get_poses_host(slam_pf *pf, float *x, float *y, float *theta);
int slam_pf_get_map_host(slam_pf *pf, float *rows /* [n_particles][5][n_landmarks] */);
/* The maps of SOME particles (a host usually wants the heaviest particle's map, not a million of them):
 * rows[k] = the landmarks of current particle particle[k] (0 <= particle[k] < n_particles, repeats allowed), pending
 * gather applied, whatever the layout; synchronises.  Sharded: collective like slam_pf_get_map_host (the exchange of
 * the last frame is completed first), indices are local. */
int slam_pf_get_map_rows_host(slam_pf *pf, const int32_t *particle, int count, float *rows /* [count][5][n_landmarks] */);

/* Inspection of a session that is on pages right now (tests, debugging; SLAM_ERR_NOT_READY when it is on rows).  Device
 * pointers into the session's own state, valid until the next slam_pf_* call that changes the layout:
 *   pool[npages][5][page_landmarks]  the pages;  table[table_rows][pages_per_particle]: page of (particle, block) for the
 *   CURRENT particles before the pending gather (rows n_particles .. table_rows - 1: staging rows of a sharded session);
 *   stamp[npages]: pages named by the current tables carry stamp_now;  freelist[]: entries [state[1], state[0]) are pages
 *   nobody names, entries [state[3], state[1]) were handed out by the last update;  state = {free, used, renewed, base}.
 * SLAM_MAP_SPLIT_PAGES: planes = 2 (a page holds mu_x | mu_y of its 32 landmarks; the covariances are the class's:
 * slam_pf_split_device_view), and the pool is two buffers: page p starts at float offset
 * p * planes * page_landmarks + (p >= half_pages ? gap_floats : 0) from `pool`.  Joint pages: planes = 5, gap_floats = 0. */
typedef struct {
    const float *pool;
    const int32_t *table, *freelist, *state;
    const uint32_t *stamp;
    uint32_t stamp_now;
    int32_t page_landmarks, pages_per_particle, table_rows;
    int64_t npages;
    int32_t planes, reserved;
    int64_t half_pages, gap_floats;
} slam_pf_paged_view;
int slam_pf_paged_device_view(slam_pf *pf, slam_pf_paged_view *out);

/* Inspection of a session that is on the split layout right now (tests, debugging; SLAM_ERR_NOT_READY otherwise).  Device
 * pointers, valid until the next slam_pf_* call: mean[rows][2][plane_stride] and cls[rows] of the CURRENT particles before the
 * pending gather; cov[..][3][plane_stride]: row c = the covariance planes of class c; live[0 .. *live_count): the classes in use
 * as of the last landmark update (a superset of those the current particles name).  SLAM_MAP_SPLIT_PAGES: mean == NULL (the
 * means are on pages: slam_pf_paged_device_view), the rest as described. */
typedef struct {
    const float *mean, *cov;
    const int32_t *cls, *live, *live_count;
    int32_t plane_stride, rows;
} slam_pf_split_view;
int slam_pf_split_device_view(slam_pf *pf, slam_pf_split_view *out);
/* ... and covx[..][2][plane_stride]: row c = the determinant terms of class c's covariances, 1 / det (P + q I) and
 * 0.5 log det (P + q I), as the next landmark update will read them (same validity as the view's pointers). */
int slam_pf_split_covx_view(slam_pf *pf, const float **covx);

/* ------------------------------------------------------------------ mapper: the reference's frame loop in one call
 * (SURVEY.md §8f rows N1 + N2).  One slam_mapper_next_frame = one iteration of the reference's loop
 * (main.c:859-969): scan clean-up, world transform, local-map crop, both rasters, both EDTs on key frames,
 * constant-velocity guess, FastMatch + FastMatch2, key-frame test and map append — with the scan, the map,
 * the local map and the grids resident on the device.  Only what the reference computes with libm (cos/sin
 * of beam angles, pose and lattice headings) and the arg-min / key-frame decisions run on the host, so the
 * pose sequence and the final map are bit-identical to the reference program's.  Uses grid slots 0 and 1 of
 * the engine.  `ranges` = one raw scan frame of `nbeams` floats (what main.c:22-30 parses from the CSV). */
typedef struct slam_mapper slam_mapper;
/* The run-time parameters the reference keeps as locals of main() and as literals: one plain struct,
 * slam_mapper_params_default fills in the reference's values. */
typedef struct {
    float fast_res[3];          /* fastResolution  {0.05, 0.05, 0.008727}    main.c:832: lattice step of FastMatch (x = y, theta) */
    float fast_res2[3];         /* fastResolution2 {0.025, 0.025, 0.004363}  main.c:833: ... of FastMatch2 */
    float border;               /* borderSize 1          main.c:834: margin of the local-map crop around the scan, metres */
    float pixel, pixel2;        /* pixelSize 0.2, pixelSize2 0.1   main.c:835-836: coarse / fine grid resolution, metres */
    float key_dt, key_dr;       /* miniUpdateDT 0.3 m, miniUpdateDR 0.0872665 rad   main.c:838-839: key-frame test, per axis */
    float range_min;            /* lidar.range_min 0.023 main.c:50 */
    float usable_range;         /* readAScan(24)         main.c:846, :863 (the reference compares with an int) */
    float edt_cap;              /* 10 cells              main.c:224 (<= 32) */
    float new_point_threshold;  /* 1.5 cells             main.c:943: a beam farther than this from the map is a new map point */
} slam_mapper_params;
void slam_mapper_params_default(slam_mapper_params *p);
/* slam_mapper_create = slam_mapper_create_ex with the defaults (params == NULL means the same) */
int slam_mapper_create(slam_engine *e, int nbeams, float angle_min, float angle_inc, slam_mapper **out);
int slam_mapper_create_ex(slam_engine *e, int nbeams, float angle_min, float angle_inc, const slam_mapper_params *params,
                          slam_mapper **out);
int slam_mapper_destroy(slam_mapper *m);
int slam_mapper_first_frame(slam_mapper *m, const float *ranges);                    /* main.c:844-858 */
int slam_mapper_next_frame(slam_mapper *m, const float *ranges, float pose_out[3]);  /* main.c:859-969 */
/* map points (main.c:982-985 writes them as "%f,%f" lines); x/y may be NULL to query the size only */
int slam_mapper_get_map_host(slam_mapper *m, float *x, float *y, int32_t capacity, int32_t *n);

/* Inspection of a mapper (tests, debugging).  Device pointers into the mapper's own state, valid until the next
 * slam_mapper_* call, and a copy of its host state.  Synchronises nothing: call slam_engine_sync first.
 *   bx/by[0 .. counts[0])  the cleaned scan, sensor frame;  tx/ty: its world points as of the last frame that made them
 *   mx/my[0 .. counts[1])  the map (map_cap floats each);   lx/ly[0 .. counts[2]): the local map of the last rebuild
 *   counts                 {nscan, msize, lsize}
 *   occ[k], edt[k]         coarse (k = 0) and fine (k = 1) occupancy grid and distance transform, ld[k] x ld[k] storage
 *   meta[2]                the two grids' records as the rasteriser wrote them
 *   hits[0 .. nbeams)      the matcher's persistent hit scratch;  nhits: the best candidate's count (host)
 *   pose, prev, map_pose, mini_updated, frame: the reference's loop locals (main.c:844-969) */
typedef struct {
    const float *bx, *by, *tx, *ty, *mx, *my, *lx, *ly;
    const int32_t *counts;
    const int32_t *occ[2];
    const float *edt[2];
    int32_t ld[2];
    const slam_grid_meta *meta;
    const float *hits;
    int32_t nhits;
    float pose[3], prev[3], map_pose[3];
    int32_t mini_updated, frame, map_cap, nbeams;
} slam_mapper_view;
int slam_mapper_device_view(const slam_mapper *m, slam_mapper_view *out);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_HIP_H */
