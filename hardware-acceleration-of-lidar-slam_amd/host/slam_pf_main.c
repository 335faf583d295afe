/*
 * slam_pf_main — particle-filter form of the reference's SLAM program, host code in C, one or several GPUs.
 *
 * Same scan-frame CSV input and the same pose / map outputs as Subsystem_1/main_accelerated.c
 * ("scan N", "pose = %f  %f  %f" on stdout, "%f,%f" map lines; main.c:22-30, :860, :965, :982-985), and the
 * same map machinery (local map, two rasters, EDT on key frames; main.c:865-872, :928-961).  What changes
 * is the pose search: instead of the reference's two 27-pose lattice sweeps (main.c:901-918) every frame
 * runs one particle-filter step on the GPU — N particles are moved by the constant-velocity increment of
 * main.c:875-898 plus noise, each is scored against the fine EDT with the reference's own score function,
 * weights are normalised and the population is resampled; the frame's pose is the posterior mean of the
 * population (exact fixed-point sums on the device: the plain mean of a resampled, hence equally weighted population,
 * the weighted mean of a frame that --ess kept) — or, with estimator "best", the heaviest particle.
 * All of it goes through the C ABI (slam_pf_* in include/slam_hip.h); no HIP or RCCL type appears here.
 *
 * Several GPUs: the accelerator handle is created once per GPU and threaded through, the shape of the reference's
 * FPGA host (Submodule_2/Hadrware_acclereated.cpp:842-845, 284): one host thread per GPU owns one engine, one
 * communicator and one sharded session, runs this same frame loop, and the engine issues every exchange between
 * the GPUs itself (RCCL over xGMI).  The population is split in contiguous blocks; the output does not depend on
 * the number of GPUs (bit for bit: pose log and map file).
 *
 * usage: slam_pf_main dataset.csv frames beams map_out.csv particles [seed [mean|best]]
 *                     [--gpus N] [--transport rccl|local] [--same-device] [--ess F] [--refine SWEEPS [--refine-res T R]]
 *                     [--landmarks L [--assoc GATE NEW_GATE [--merge GATE] [--assoc-weight LOG_NEW LOG_CLUTTER LOG_MISS] [--prune HIT MISS CMAX RANGE [--prune-sight BINS MARGIN] [--prune-fov EDGE]]
 *                      [--detect [JUMP GUARD WIDTH RANGE MIN MAX WRAP] [--pole-radius R [TOL]] [--range-noise RV BV [LV]]]]
 *                     [--landmarks-out FILE]]
 *                     [--known-map FILE GATE MAP_VAR [LOG_CLUTTER] [--detect [..] [--pole-radius R [TOL]] [--range-noise RV BV [LV]]]
 *                      [--known-reseed FRACTION [EVERY] | --known-reseed-pairs FRACTION TOL MIN_SEP [EVERY]]]
 *                     [--spread-out FILE] [--modes-out FILE CELL HBINS M]
 *   particles      the whole population (a multiple of N)
 *   --ess F        ESS-gated resampling: resample only in frames whose effective sample size is below F * N
 *   --refine SWEEPS  scan-match refinement of every particle (slam_pf_refine_set): SWEEPS (1..16) sweeps of the reference's
 *                  27-pose lattice around each motion sample, the particle weighted at the pose it ends on
 *   --refine-res T R  its steps in metres and radians (default: the reference's fastResolution2, 0.025 0.004363; main.c:833)
 *   --transport    rccl (default when N > 1): RCCL, one GPU per rank.  local: the in-process transport.
 *   --same-device  every rank on device 0 (only with the local transport; RCCL refuses two ranks on one GPU)
 *   --landmarks L  the session is made on rows (SLAM_MAP_ROWS) with L landmark slots per particle; one GPU.  Without it the
 *                  filter keeps no landmarks and the options below are refused
 *   --assoc GATE NEW_GATE  data association (slam_pf_assoc_set, create = 1): frames read the engine's detections.  Together
 *                  with --meas-cov and --landmarks: association under that covariance (slam_pf_assoc_cov_set, one call for both)
 *   --prune HIT MISS CMAX RANGE  existence evidence and pruning of clutter landmarks (slam_pf_prune_set)
 *   --prune-sight BINS MARGIN  only with --prune: a landmark behind what the frame's scan hit in its direction (BINS directions, a
 *                  power of two in 32 .. 1024; nearer than the landmark by more than MARGIN metres) takes no miss (slam_pf_prune_sight_set)
 *   --prune-fov EDGE  only with --prune: a landmark whose direction lies outside the lidar's arc — the first to the last beam angle
 *                  of the scan, narrowed by EDGE >= 0 radians at both ends — takes no miss (slam_pf_prune_fov_set)
 *   --merge GATE   only with --assoc: behind every frame's update a landmark that took no detection and lies within GATE (the
 *                  Mahalanobis term under the sum of the two covariances) of one that took one is fused into it and its slot
 *                  freed — duplicates of one pole become one landmark (slam_pf_merge_set)
 *   --assoc-weight LOG_NEW LOG_CLUTTER LOG_MISS  only with --assoc: every detection that starts a landmark adds LOG_NEW to its
 *                  particle's log-likelihood, every dropped one LOG_CLUTTER and — with --prune — every landmark in view that took
 *                  none LOG_MISS; each finite and <= 0 (slam_pf_assoc_weight_set)
 *   --detect [JUMP GUARD WIDTH RANGE MIN MAX WRAP]  the detector (slam_pf_detect_set; no values: slam_detect_params_default):
 *                  every frame makes its detections from its own scan, so the landmark map grows from nothing but lidar frames
 *   --range-noise RANGE_VAR BEARING_VAR [LATERAL_VAR]  only with --detect and --assoc or --known-map: the detector's noise model
 *                  (slam_pf_detect_noise_set) and association under the covariance each detection carries
 *                  (slam_pf_assoc_detcov_set; with --known-map: slam_pf_known_map_detcov_set)
 *   --pole-radius R [TOL]  only with --detect: a detection is the centre of the circle of radius R fitted to its segment, not the
 *                  segment's centroid, and segments more spread out than such a circle (by more than TOL, default 0) are no
 *                  detections (slam_pf_detect_fit_set)
 *   --landmarks-out FILE  at the end, the seen landmarks (P_xx >= 0) of the heaviest particle as "%f,%f" lines
 *   --known-map FILE GATE MAP_VAR [LOG_CLUTTER]  localisation in a known landmark map (slam_pf_known_map_set): FILE holds "%f,%f"
 *                  lines as --landmarks-out writes them, every landmark gets P = MAP_VAR * I (MAP_VAR >= 0); the filter keeps no
 *                  landmarks of its own, every frame associates its detections (--detect) with this one map within GATE, weighs
 *                  each particle with the matched pairs' likelihood and adds LOG_CLUTTER (<= 0, default 0) per unmatched
 *                  detection.  With --range-noise every detection is weighed under its own covariance instead of the session's
 *                  meas_var * I (slam_pf_known_map_detcov_set).  One GPU; not with --landmarks or --meas-cov
 *   --known-miss LOG_MISS VIEW_RANGE [--known-miss-fov EDGE] [--known-miss-sight BINS MARGIN]  only with --known-map
 *                  (slam_pf_known_map_miss_set): a landmark of the map within VIEW_RANGE metres of a particle's pose that no detection
 *                  matched costs the particle LOG_MISS (<= 0) — unless it lies outside the lidar's arc (--known-miss-fov: the first
 *                  to the last beam angle, narrowed by EDGE radians at each end) or behind what the scan hit (--known-miss-sight)
 *   --known-reseed FRACTION [EVERY]  only with --known-map: behind every EVERY-th observing frame (default 1), once the frame's
 *                  outputs are read, FRACTION (in (0, 1]) of the particles is replaced by pose proposals at which one of the
 *                  frame's detections coincides with one landmark of the map (slam_pf_known_map_reseed) — what brings back a cloud
 *                  that settled on a wrong pose; the frame's line then ends in "  reseed = REPLACED NOT_REPLACED"
 *   --known-reseed-pairs FRACTION TOL MIN_SEP [EVERY]  only with --known-map, not with --known-reseed: the same with proposals
 *                  from PAIRS of detections (slam_pf_known_map_reseed_pairs) — two detections at least MIN_SEP metres apart on
 *                  two landmarks whose distance is the detections' within TOL metres (0 <= TOL < MIN_SEP) fix the heading as
 *                  well; a frame with fewer than two detections is skipped (counts 0); the frame's line then ends in
 *                  "  reseed-pairs = REPLACED EMPTY TOO_CLOSE NO_PARTNER"
 *   --spread-out FILE  every frame also asks for the spread of the population about its mean (slam_pf_spread, around the same
 *                  predicted heading) and writes one line to FILE: the frame number, the six entries of the covariance over
 *                  (x, y, sin dtheta) — xx, xy, yy, xs, ys, ss — and the length of the mean heading vector, comma-separated, each
 *                  number as %.9g (enough to give back its binary32).  A small spread says that the particles agree, not that
 *                  they are right.  Every other output stays byte for byte what it is without the flag
 *   --modes-out FILE CELL HBINS M  every frame also asks for the modes of the population (slam_pf_modes, around the same
 *                  predicted heading: cells of CELL metres and HBINS heading bins, at most M modes) and writes one line to FILE:
 *                  the frame number, the number of modes, the number of occupied cells, then x y theta mass per mode, heaviest
 *                  first, space-separated, each number as %.9g.  One GPU: refused with --gpus N > 1 or --transport.  Every
 *                  other output stays byte for byte what it is without the flag
 */
#define _POSIX_C_SOURCE 200809L
#include <math.h>
#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "slam_frontend.h"

static double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

typedef struct {
    /* the run */
    const char *dataset, *map_out;
    int frames, beams, particles_total, use_mean;
    unsigned long long seed;
    float ess_frac;        /* --ess F: resample only when the effective sample size is below F * N (0: every frame) */
    int refine_sweeps;     /* --refine SWEEPS (0: off) */
    float refine_res[2];   /* --refine-res T R */
    int use_meas_cov;      /* --meas-cov qxx qxy qyy: the session is made on rows and given this measurement covariance */
    float meas_cov[3];
    int landmarks;         /* --landmarks L (0: the filter keeps no landmarks) */
    int use_assoc;         /* --assoc GATE NEW_GATE */
    float assoc_gate[2];
    int use_prune;         /* --prune HIT MISS CMAX RANGE */
    int prune[3];
    float prune_range;
    int use_sight;         /* --prune-sight BINS MARGIN: only with --prune */
    int sight_bins;
    float sight_margin;
    int use_fov;           /* --prune-fov EDGE: only with --prune */
    float fov_edge;
    int use_merge;         /* --merge GATE: only with --assoc */
    float merge_gate;
    int use_assoc_weight;  /* --assoc-weight LOG_NEW LOG_CLUTTER LOG_MISS: only with --assoc */
    float assoc_weight[3];
    int use_detect;        /* --detect [JUMP GUARD WIDTH RANGE MIN MAX WRAP] */
    slam_detect_params detect;
    int use_fit;           /* --pole-radius R [TOL] */
    slam_detect_fit fit;
    int use_noise;         /* --range-noise RANGE_VAR BEARING_VAR [LATERAL_VAR]: only with --detect */
    slam_detect_noise noise;
    const char *landmarks_out;   /* --landmarks-out FILE */
    const char *spread_out;      /* --spread-out FILE */
    FILE *spread;                /* ... opened in main, before any rank runs; rank 0 writes */
    const char *modes_out;       /* --modes-out FILE CELL HBINS M */
    FILE *modes;
    float modes_cell;
    int modes_hbins, modes_max;
    const char *known_map;       /* --known-map FILE GATE MAP_VAR [LOG_CLUTTER] */
    float known_gate, known_var, known_log_clutter;
    float *known_rows;           /* [5][known_n]: the file's points, P = MAP_VAR * I */
    int use_known_miss;          /* --known-miss LOG_MISS VIEW_RANGE: only with --known-map */
    float known_log_miss, known_view_range;
    int known_miss_fov;          /* --known-miss-fov EDGE: only with --known-miss */
    float known_miss_edge;
    int known_miss_bins;         /* --known-miss-sight BINS MARGIN: only with --known-miss; 0: off */
    float known_miss_margin;
    int known_n;
    int use_known_reseed;        /* --known-reseed FRACTION [EVERY]: only with --known-map */
    float known_reseed_fraction;
    int known_reseed_every;
    int use_known_reseed_pairs;  /* --known-reseed-pairs FRACTION TOL MIN_SEP [EVERY]: FRACTION and EVERY in the two fields above */
    float known_reseed_tol, known_reseed_min_sep;
    /* the ranks */
    int world, use_rccl, same_device;
    uint8_t comm_id[SLAM_COMM_ID_BYTES];
    slam_local_group *group;
} run_t;

typedef struct {
    run_t *run;
    int rank, rc;
} rank_t;

#define CHECK(call)                                                                                               \
    do {                                                                                                          \
        int rc__ = (call);                                                                                        \
        if (rc__ != SLAM_OK) {                                                                                    \
            fprintf(stderr, "rank %d: %s failed: %s (%s)\n", rank, #call, slam_status_string(rc__),                \
                    eng ? slam_last_error(eng) : "");                                                             \
            goto fail;                                                                                            \
        }                                                                                                         \
    } while (0)

static void *rank_main(void *arg)
{
    rank_t *me = (rank_t *)arg;
    run_t *run = me->run;
    const int rank = me->rank, world = run->world;
    const int beams = run->beams, frames = run->frames;
    const int n = run->particles_total / world, n_total = run->particles_total;
    const float border = 1, pixel_coarse = 0.2f, pixel_fine = 0.1f;   /* main.c:834-836 */
    const float key_dt = 0.3f, key_dr = 0.0872665f, edt_cap = 10;     /* main.c:838-839, :224 */
    slam_engine *eng = NULL;
    slam_comm *comm = NULL;
    slam_pf *pf = NULL;
    FILE *in = NULL;
    float *hits = NULL;
    fe_scan scan = { 0 };
    fe_points map = { 0 }, local = { 0 };
    fe_grid coarse = { 0 }, fine = { 0 };
    me->rc = 1;

    in = fopen(run->dataset, "r");   /* every rank reads the (small) scan stream itself: no host-side broadcast */
    if (!in) { perror(run->dataset); goto fail; }
    {
        int rc = slam_engine_create(run->same_device ? 0 : rank, &eng);
        if (rc != SLAM_OK) {
            fprintf(stderr, "rank %d: slam_engine_create: %s\n", rank, slam_status_string(rc));
            eng = NULL;
            goto fail;
        }
    }
    /* motion noise of the order of the reference's fine lattice step (0.025 m, 0.004363 rad; main.c:833) */
    /* ... and, with landmarks, a detection noise of the order of a pole's radius (0.1 m); without them meas_var is not read */
    const slam_pf_config cfg = { n, run->landmarks, { 0.01f, 0.01f, 0.002f }, run->landmarks > 0 || run->known_map ? 0.01f : 1.0f, 0.25f, run->seed, run->ess_frac,
                                 run->use_meas_cov || run->landmarks > 0 ? SLAM_MAP_ROWS : SLAM_MAP_AUTO };
    if (world > 1 || run->use_rccl || run->group) {
        if (run->group) CHECK(slam_comm_create_local(eng, run->group, rank, &comm));
        else CHECK(slam_comm_create_rccl(eng, rank, world, run->comm_id, &comm));
        CHECK(slam_pf_create_sharded(eng, &cfg, comm, 0, &pf));
    } else {
        CHECK(slam_pf_create(eng, &cfg, &pf));
    }
    if (run->refine_sweeps) CHECK(slam_pf_refine_set(pf, run->refine_res[0], run->refine_res[1], run->refine_sweeps));
    /* --assoc and --meas-cov with landmarks: one switch sets covariance and gates together (each of the two separate switches
     * refuses the other) */
    const int assoc_cov = run->use_assoc && run->use_meas_cov && run->landmarks > 0;
    if (assoc_cov) CHECK(slam_pf_assoc_cov_set(pf, run->meas_cov, run->assoc_gate[0], run->assoc_gate[1], 1));
    if (run->use_meas_cov && !assoc_cov) {
        /* Without --landmarks this program's filter keeps none (n_landmarks = 0): a session without them has no covariance to
         * apply the matrix to and says so (the values themselves were checked in main).  That is reported, not fatal: the run
         * goes on as it would on rows.  With landmarks the call's result is checked. */
        const int rc = slam_pf_meas_cov_set(pf, run->meas_cov);
        if (cfg.n_landmarks > 0) CHECK(rc);
        else if (rank == 0) fprintf(stderr, "--meas-cov has no effect here: %s\n", slam_last_error(eng));
    }
    /* the landmark pipeline: association reads detections, the detector makes them from each frame's scan */
    if (run->use_assoc && !assoc_cov && !run->use_noise) CHECK(slam_pf_assoc_set(pf, run->assoc_gate[0], run->assoc_gate[1], 1));
    /* --range-noise: every detection carries its own covariance, association and update run under it */
    if (run->use_assoc && !assoc_cov && run->use_noise) CHECK(slam_pf_assoc_detcov_set(pf, run->assoc_gate[0], run->assoc_gate[1], 1));
    if (run->use_prune) CHECK(slam_pf_prune_set(pf, run->prune[0], run->prune[1], run->prune[2], run->prune_range));
    if (run->use_sight) CHECK(slam_pf_prune_sight_set(pf, run->sight_bins, run->sight_margin));
    if (run->use_merge) CHECK(slam_pf_merge_set(pf, run->merge_gate));
    if (run->use_assoc_weight) CHECK(slam_pf_assoc_weight_set(pf, run->assoc_weight[0], run->assoc_weight[1], run->assoc_weight[2], 1));
    /* --range-noise: the form of the stage that weighs every detection under the covariance the detector's model gives it */
    if (run->known_map)
        CHECK((run->use_noise ? slam_pf_known_map_detcov_set : slam_pf_known_map_set)(pf, run->known_rows, run->known_n, run->known_gate,
                                                                                    run->known_log_clutter));
    if (run->use_detect) CHECK(slam_pf_detect_noise_set(pf, &run->detect, run->use_fit ? &run->fit : NULL, run->use_noise ? &run->noise : NULL));
    const int observe = (run->known_map || (run->landmarks > 0 && run->use_assoc)) && run->use_detect;   /* else: no frame has observations */
    if (fe_scan_init(&scan, beams, -2.351831f, 0.004363f) || fe_points_init(&map, FE_MAP_CAPACITY + beams) ||
        fe_points_init(&local, FE_LOCAL_CAPACITY) || fe_grid_init(&coarse, FE_COARSE_LD) || fe_grid_init(&fine, FE_FINE_LD) ||
        !(hits = (float *)calloc((size_t)beams + 1, sizeof(float)))) {
        fprintf(stderr, "rank %d: out of memory\n", rank);
        goto fail;
    }
    /* --prune-fov: the arc is the scan's own, its first and its last beam angle */
    if (run->use_fov) CHECK(slam_pf_prune_fov_set(pf, 1, scan.angle[0], scan.angle[beams - 1], run->fov_edge));
    /* --known-miss: the arc, if asked for, likewise */
    if (run->use_known_miss)
        CHECK(slam_pf_known_map_miss_set(pf, run->known_log_miss, run->known_view_range, run->known_miss_fov, scan.angle[0], scan.angle[beams - 1],
                                         run->known_miss_edge, run->known_miss_bins, run->known_miss_margin));
    int32_t nhits = 0;
    double t_step = 0;
    const double t_begin = now_s();

    float pose[3] = { 0, 0, 0 }, prev[3] = { 0, 0, 0 };
    fe_read_frame(in, &scan);
    fe_clean(&scan, 0.023f, 24);
    fe_to_world(&scan, pose);
    memcpy(map.x, scan.wx, sizeof(float) * (size_t)scan.nscan);
    memcpy(map.y, scan.wy, sizeof(float) * (size_t)scan.nscan);
    map.size = scan.nscan;
    memcpy(map.pose, pose, sizeof pose);
    CHECK(slam_pf_reset(pf, pose));
    int mini_updated = 1;
    int observing_frames = 0;   /* --known-reseed: every EVERY-th of them is followed by a reseed */

    for (int k = 1; k < frames; ++k) {
        if (rank == 0) printf("scan %d\n", k + 1);
        fe_read_frame(in, &scan);
        fe_clean(&scan, 0.023f, 24);
        CHECK(slam_scan_upload_host(eng, scan.bx, scan.by, scan.nscan));
        int in_world = 0;
        if (mini_updated) {   /* map, rasters and EDTs are replicated on every GPU (<= 16 MiB) */
            fe_to_world(&scan, pose);
            in_world = 1;
            fe_crop(&map, &scan, border, &local);
            if (fe_rasterise(&local, pixel_coarse, &coarse) || fe_rasterise(&local, pixel_fine, &fine)) {
                fprintf(stderr, "frame %d: map extent exceeds the grids\n", k + 1);
                goto fail;
            }
            CHECK(slam_grid_upload_host(eng, 0, coarse.cell, &coarse.meta, edt_cap, NULL));
            CHECK(slam_grid_upload_host(eng, 1, fine.cell, &fine.meta, edt_cap, NULL));
        }
        /* constant-velocity increment (main.c:875-898) drives the motion model of every particle */
        float dp[3];
        for (int a = 0; a < 3; ++a) dp[a] = k > 1 ? pose[a] - prev[a] : 0.0f;
        const double t0 = now_s();
        CHECK(slam_pf_step(pf, 1, dp, observe));
        float best[3];
        if (run->use_mean) {
            /* posterior mean over ALL ranks' particles = plain mean of a resampled population, weighted mean of one that the
             * resample gate (--ess) kept: exact integer sums made on the device (slam_pf_mean), so the result does not depend
             * on the number of GPUs.  Headings are averaged on the
             * circle, around the predicted heading, so that a population straddling +-pi does not average to nonsense and
             * theta stays unwrapped (the reference never normalises angles). */
            CHECK(slam_pf_mean(pf, pose[2] + dp[2], best));
        } else {
            CHECK(slam_pf_best(pf, best, NULL, NULL));   /* sharded: the heaviest of the whole population, on every rank */
        }
        t_step += now_s() - t0;
        if (run->spread_out) {   /* collective on several GPUs: every rank asks, rank 0 writes */
            float sp[3], cov[6], heading_r;
            CHECK(slam_pf_spread(pf, pose[2] + dp[2], sp, cov, &heading_r));
            if (rank == 0)
                fprintf(run->spread, "%d,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g\n", k + 1, (double)cov[0], (double)cov[1], (double)cov[2],
                        (double)cov[3], (double)cov[4], (double)cov[5], (double)heading_r);
        }
        if (run->modes_out) {   /* one GPU only (main refuses the rest) */
            slam_pf_mode md[8];
            int n_modes = 0, cells = 0;
            CHECK(slam_pf_modes(pf, pose[2] + dp[2], run->modes_cell, run->modes_hbins, run->modes_max, md, &n_modes, &cells));
            fprintf(run->modes, "%d %d %d", k + 1, n_modes, cells);
            for (int m = 0; m < n_modes; ++m)
                fprintf(run->modes, " %.9g %.9g %.9g %.9g", (double)md[m].pose[0], (double)md[m].pose[1], (double)md[m].pose[2],
                        (double)md[m].mass);
            fputc('\n', run->modes);
        }
        memcpy(prev, pose, sizeof prev);
        memcpy(pose, best, sizeof pose);

        if (fabsf(pose[0] - map.pose[0]) > key_dt || fabsf(pose[1] - map.pose[1]) > key_dt ||
            fabsf(pose[2] - map.pose[2]) > key_dr) {
            mini_updated = 1;
            if (!in_world) fe_to_world(&scan, pose);
            /* hits of the frame's pose on the fine grid (the reference uses its matcher scratch here, main.c:942-948) */
            CHECK(slam_pose_hits_host(eng, 1, pose[0], pose[1], cosf(pose[2]), sinf(pose[2]), hits, &nhits));
            int added = 0;
            for (int j = 0; j < nhits; ++j)
                if (hits[j] > 1.5 && map.size + added < map.capacity) {
                    map.x[map.size + added] = scan.wx[j];
                    map.y[map.size + added] = scan.wy[j];
                    ++added;
                }
            map.size += added;
            memcpy(map.pose, pose, sizeof pose);
        } else {
            mini_updated = 0;
        }
        if (run->use_known_reseed && observe) {   /* the frame's outputs are read: now the proposals for the next one */
            int32_t reseed[2] = { 0, 0 };
            const int due = ++observing_frames % run->known_reseed_every == 0;
            if (due) CHECK(slam_pf_known_map_reseed(pf, run->known_reseed_fraction, reseed));
            if (rank == 0) printf("pose = %f  %f  %f  reseed = %d %d\n", pose[0], pose[1], pose[2], (int)reseed[0], (int)reseed[1]);
        } else if (run->use_known_reseed_pairs && observe) {
            int32_t reseed[4] = { 0, 0, 0, 0 };
            const int due = ++observing_frames % run->known_reseed_every == 0;
            if (due)
                CHECK(slam_pf_known_map_reseed_pairs(pf, run->known_reseed_fraction, run->known_reseed_tol, run->known_reseed_min_sep, reseed));
            if (rank == 0)
                printf("pose = %f  %f  %f  reseed-pairs = %d %d %d %d\n", pose[0], pose[1], pose[2], (int)reseed[0], (int)reseed[1],
                       (int)reseed[2], (int)reseed[3]);
        } else if (rank == 0) printf("pose = %f  %f  %f\n", pose[0], pose[1], pose[2]);
    }
    if (rank == 0) {
        const double wall = now_s() - t_begin;
        fprintf(stderr, "frames %d  particles %d  gpus %d  wall %.6f s  pf steps %.6f s (%.3e particle-updates/s)\n", frames,
                n_total, world, wall, t_step, (double)n_total * (frames - 1) / t_step);
        FILE *out = fopen(run->map_out, "w");
        if (!out) { perror(run->map_out); goto fail; }
        for (int j = 0; j < map.size; ++j) fprintf(out, "%f,%f\n", map.x[j], map.y[j]);
        fclose(out);
    }
    if (rank == 0 && run->landmarks_out) {
        /* the heaviest particle of the last frame is named by its index BEFORE that frame's resample; the rows that can be
         * asked for are those of the CURRENT particles: take the first one that carries its pose (an offspring of it) */
        const int L = run->landmarks;
        float bp[3], *px = (float *)malloc(sizeof(float) * 3 * (size_t)n), *row = (float *)malloc(sizeof(float) * 5 * (size_t)L);
        int32_t sel = 0;
        int rc_out = px && row ? SLAM_OK : SLAM_ERR_CAPACITY;
        if (rc_out == SLAM_OK) rc_out = slam_pf_best(pf, bp, NULL, NULL);
        if (rc_out == SLAM_OK) rc_out = slam_pf_get_poses_host(pf, px, px + n, px + 2 * (size_t)n);
        if (rc_out == SLAM_OK) {
            int found = 0;
            for (int j = 0; j < n && !found; ++j)
                if (px[j] == bp[0] && px[n + j] == bp[1] && px[2 * (size_t)n + j] == bp[2]) { sel = j; found = 1; }
            if (!found) fprintf(stderr, "--landmarks-out: the heaviest particle left no offspring; writing particle 0's map\n");
            rc_out = slam_pf_get_map_rows_host(pf, &sel, 1, row);
        }
        FILE *out = rc_out == SLAM_OK ? fopen(run->landmarks_out, "w") : NULL;
        if (out) {
            int seen = 0;
            for (int l = 0; l < L; ++l)
                if (!(row[2 * L + l] < 0.0f)) { fprintf(out, "%f,%f\n", row[l], row[L + l]); ++seen; }
            fclose(out);
            fprintf(stderr, "landmarks %d of %d slots\n", seen, L);
        }
        free(px);
        free(row);
        if (rc_out != SLAM_OK) CHECK(rc_out);
        if (!out) { perror(run->landmarks_out); goto fail; }
    }
    me->rc = 0;
fail:
    if (me->rc && comm) slam_comm_abort(comm);   /* the other ranks must not wait for this one: their calls fail with SLAM_ERR_COMM */
    free(hits);
    fe_grid_free(&coarse); fe_grid_free(&fine);
    fe_points_free(&map); fe_points_free(&local);
    fe_scan_free(&scan);
    if (in) fclose(in);
    slam_pf_destroy(pf);
    slam_comm_destroy(comm);
    slam_engine_destroy(eng);
    return NULL;
}

int main(int argc, char **argv)
{
    run_t run;
    memset(&run, 0, sizeof run);
    run.world = 1;
    run.use_mean = 1;
    run.seed = 1;
    run.refine_res[0] = 0.025f;   /* fastResolution2 (main.c:833) */
    run.refine_res[1] = 0.004363f;
    const char *pos[8];
    int npos = 0, transport_given = 0, use_local = 0;
    for (int a = 1; a < argc; ++a) {
        if (!strcmp(argv[a], "--gpus") && a + 1 < argc) run.world = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--transport") && a + 1 < argc) { use_local = !strcmp(argv[++a], "local"); transport_given = 1; }
        else if (!strcmp(argv[a], "--same-device")) run.same_device = 1;
        else if (!strcmp(argv[a], "--ess") && a + 1 < argc) run.ess_frac = (float)atof(argv[++a]);
        else if (!strcmp(argv[a], "--refine") && a + 1 < argc) run.refine_sweeps = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--refine-res") && a + 2 < argc) {
            run.refine_res[0] = (float)atof(argv[++a]);
            run.refine_res[1] = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--meas-cov") && a + 3 < argc) {
            run.use_meas_cov = 1;
            for (int k = 0; k < 3; ++k) run.meas_cov[k] = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--landmarks") && a + 1 < argc) run.landmarks = atoi(argv[++a]);
        else if (!strcmp(argv[a], "--assoc") && a + 2 < argc) {
            run.use_assoc = 1;
            for (int k = 0; k < 2; ++k) run.assoc_gate[k] = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--prune") && a + 4 < argc) {
            run.use_prune = 1;
            for (int k = 0; k < 3; ++k) run.prune[k] = atoi(argv[++a]);
            run.prune_range = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--prune-sight") && a + 2 < argc) {
            run.use_sight = 1;
            run.sight_bins = atoi(argv[++a]);
            run.sight_margin = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--prune-fov") && a + 1 < argc) {
            char *end = NULL;
            run.use_fov = 1;
            run.fov_edge = strtof(argv[++a], &end);
            if (end == argv[a] || *end || !isfinite(run.fov_edge) || run.fov_edge < 0.0f) {
                fprintf(stderr, "--prune-fov %s: EDGE must be a finite number of radians >= 0\n", argv[a]);
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--merge") && a + 1 < argc) {
            char *end = NULL;
            run.use_merge = 1;
            run.merge_gate = strtof(argv[++a], &end);
            if (end == argv[a] || *end || !isfinite(run.merge_gate) || run.merge_gate <= 0.0f) {
                fprintf(stderr, "--merge %s: GATE must be a finite number > 0\n", argv[a]);
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--assoc-weight") && a + 3 < argc) {
            run.use_assoc_weight = 1;
            for (int k = 0; k < 3; ++k) {
                char *end = NULL;
                run.assoc_weight[k] = strtof(argv[++a], &end);
                if (end == argv[a] || *end || !isfinite(run.assoc_weight[k]) || run.assoc_weight[k] > 0.0f) {
                    fprintf(stderr, "--assoc-weight %s: LOG_NEW, LOG_CLUTTER and LOG_MISS must be finite numbers <= 0\n", argv[a]);
                    return 2;
                }
            }
        }
        else if (!strcmp(argv[a], "--detect")) {
            run.use_detect = 1;
            slam_detect_params_default(&run.detect);
            /* seven values follow, or none: a value is whatever starts like a number */
            int have = 0;
            while (have < 7 && a + 1 + have < argc && strchr("0123456789.+-", argv[a + 1 + have][0]) && strncmp(argv[a + 1 + have], "--", 2))
                ++have;
            if (have == 7) {
                run.detect.jump = (float)atof(argv[a + 1]);
                run.detect.guard = (float)atof(argv[a + 2]);
                run.detect.max_width = (float)atof(argv[a + 3]);
                run.detect.max_range = (float)atof(argv[a + 4]);
                run.detect.min_points = atoi(argv[a + 5]);
                run.detect.max_points = atoi(argv[a + 6]);
                run.detect.wrap = atoi(argv[a + 7]);
                a += 7;
            }
        }
        else if (!strcmp(argv[a], "--pole-radius") && a + 1 < argc) {
            run.use_fit = 1;
            slam_detect_fit_default(&run.fit);
            run.fit.radius = (float)atof(argv[++a]);
            if (a + 1 < argc && strchr("0123456789.+", argv[a + 1][0])) run.fit.spread_tol = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--range-noise") && a + 2 < argc) {
            run.use_noise = 1;
            run.noise.range_var = (float)atof(argv[++a]);
            run.noise.bearing_var = (float)atof(argv[++a]);
            run.noise.lateral_var = 0.0f;
            if (a + 1 < argc && strchr("0123456789.+", argv[a + 1][0])) run.noise.lateral_var = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--landmarks-out") && a + 1 < argc) run.landmarks_out = argv[++a];
        else if (!strcmp(argv[a], "--spread-out") && a + 1 < argc) run.spread_out = argv[++a];
        else if (!strcmp(argv[a], "--modes-out") && a + 4 < argc) {
            run.modes_out = argv[++a];
            run.modes_cell = (float)atof(argv[++a]);
            run.modes_hbins = atoi(argv[++a]);
            run.modes_max = atoi(argv[++a]);
        }
        else if (!strcmp(argv[a], "--known-miss") && a + 2 < argc) {
            run.use_known_miss = 1;
            run.known_log_miss = (float)atof(argv[++a]);
            run.known_view_range = (float)atof(argv[++a]);
            if (!isfinite(run.known_log_miss) || run.known_log_miss > 0.0f || !isfinite(run.known_view_range) || run.known_view_range <= 0.0f) {
                fprintf(stderr, "--known-miss: LOG_MISS must be a finite number <= 0 and VIEW_RANGE a finite number > 0\n");
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--known-miss-fov") && a + 1 < argc) {
            run.known_miss_fov = 1;
            run.known_miss_edge = (float)atof(argv[++a]);
            if (!isfinite(run.known_miss_edge) || run.known_miss_edge < 0.0f) {
                fprintf(stderr, "--known-miss-fov %s: EDGE must be a finite number of radians >= 0\n", argv[a]);
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--known-miss-sight") && a + 2 < argc) {
            run.known_miss_bins = atoi(argv[++a]);
            run.known_miss_margin = (float)atof(argv[++a]);
        }
        else if (!strcmp(argv[a], "--known-reseed") && a + 1 < argc) {
            run.use_known_reseed = 1;
            run.known_reseed_fraction = (float)atof(argv[++a]);
            run.known_reseed_every = 1;
            if (a + 1 < argc && strchr("0123456789+", argv[a + 1][0])) run.known_reseed_every = atoi(argv[++a]);
            if (!(run.known_reseed_fraction > 0.0f && run.known_reseed_fraction <= 1.0f) || run.known_reseed_every < 1) {
                fprintf(stderr, "--known-reseed: FRACTION must lie in (0, 1] and EVERY must be a whole number >= 1\n");
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--known-reseed-pairs") && a + 3 < argc) {
            run.use_known_reseed_pairs = 1;
            run.known_reseed_fraction = (float)atof(argv[++a]);
            run.known_reseed_tol = (float)atof(argv[++a]);
            run.known_reseed_min_sep = (float)atof(argv[++a]);
            run.known_reseed_every = 1;
            if (a + 1 < argc && strchr("0123456789+", argv[a + 1][0])) run.known_reseed_every = atoi(argv[++a]);
            if (!(run.known_reseed_fraction > 0.0f && run.known_reseed_fraction <= 1.0f) || run.known_reseed_every < 1 ||
                !(run.known_reseed_tol >= 0.0f) || !(run.known_reseed_min_sep > run.known_reseed_tol) || !(run.known_reseed_min_sep < 1e30f)) {
                fprintf(stderr, "--known-reseed-pairs: FRACTION must lie in (0, 1], 0 <= TOL < MIN_SEP, and EVERY must be a whole number >= 1\n");
                return 2;
            }
        }
        else if (!strcmp(argv[a], "--known-map") && a + 3 < argc) {
            run.known_map = argv[++a];
            float *v[3] = { &run.known_gate, &run.known_var, &run.known_log_clutter };
            const int given = a + 3 < argc && strchr("0123456789.+-", argv[a + 3][0]) && strncmp(argv[a + 3], "--", 2) ? 3 : 2;
            for (int k = 0; k < given; ++k) {
                char *end = NULL;
                *v[k] = strtof(argv[++a], &end);
                if (end == argv[a] || *end || !isfinite(*v[k]) || (k == 0 && *v[k] <= 0.0f) || (k == 1 && *v[k] < 0.0f) || (k == 2 && *v[k] > 0.0f)) {
                    fprintf(stderr, "--known-map %s: GATE must be a finite number > 0, MAP_VAR >= 0 and LOG_CLUTTER <= 0\n", argv[a]);
                    return 2;
                }
            }
        }
        else if (npos < 8) pos[npos++] = argv[a];
    }
    const int landmark_options = run.use_assoc || run.use_prune || (run.use_detect && !run.known_map) || run.landmarks_out != NULL;
    if (npos < 5 || (run.modes_out && (run.world > 1 || transport_given)) || (run.known_map && (run.landmarks > 0 || run.world > 1 || run.use_meas_cov)) || run.world < 1 || run.world > 16 || run.refine_sweeps < 0 || run.refine_sweeps > 16 || run.landmarks < 0 ||
        (landmark_options && run.landmarks == 0) || (run.landmarks > 0 && run.world > 1) || (run.use_fit && !run.use_detect) || (run.use_sight && !run.use_prune) || (run.use_fov && !run.use_prune) || (run.use_merge && !run.use_assoc) || (run.use_assoc_weight && !run.use_assoc) || (run.use_known_miss && !run.known_map) || (run.use_known_reseed && !run.known_map) || (run.use_known_reseed_pairs && (!run.known_map || run.use_known_reseed)) || ((run.known_miss_fov || run.known_miss_bins) && !run.use_known_miss) ||
        (run.use_noise && (!run.use_detect || !(run.use_assoc || run.known_map) || run.use_meas_cov))) {
        fprintf(stderr, "usage: %s dataset.csv frames beams map_out.csv particles [seed [mean|best]] [--gpus N] "
                        "[--transport rccl|local] [--same-device] [--ess F] [--refine SWEEPS [--refine-res T R]] [--meas-cov QXX QXY QYY]\n"
                        "  [--landmarks L [--assoc GATE NEW_GATE [--merge GATE] [--assoc-weight LOG_NEW LOG_CLUTTER LOG_MISS] [--prune HIT MISS CMAX RANGE [--prune-sight BINS MARGIN] [--prune-fov EDGE]] [--detect [JUMP GUARD WIDTH RANGE MIN MAX WRAP] [--pole-radius R [TOL]] [--range-noise RANGE_VAR BEARING_VAR [LATERAL_VAR]]]] "
                        "[--landmarks-out FILE]]\n"
                        "  [--known-map FILE GATE MAP_VAR [LOG_CLUTTER] [--detect [..] [--pole-radius R [TOL]] [--range-noise RANGE_VAR BEARING_VAR [LATERAL_VAR]]]] [--spread-out FILE]\n"
                        "  [--modes-out FILE CELL HBINS M]\n"
                        "  --meas-cov: the landmark update's 2x2 sensor-frame covariance; makes the session on rows, and is otherwise inert\n"
                        "              without --landmarks; with --landmarks and --assoc the association gates and updates under it\n"
                        "  --landmarks: L landmark slots per particle on rows, one GPU; --assoc, --prune, --detect and --landmarks-out need it.\n"
                        "              With --assoc and --detect every frame makes its detections from its own scan\n"
                        "  --prune-sight BINS MARGIN: only with --prune; a landmark hidden behind what the scan hit (BINS directions, a power of\n"
                        "              two in 32 .. 1024; nearer by more than MARGIN metres) takes no miss\n"
                        "  --prune-fov EDGE: only with --prune; a landmark outside the lidar's arc (first to last beam angle, narrowed by EDGE\n"
                        "              radians at both ends) takes no miss\n"
                        "  --merge GATE: only with --assoc; a landmark that took no detection within GATE (Mahalanobis, under the sum of the two\n"
                        "              covariances) of one that took one is fused into it and its slot freed: duplicates of a pole become one\n"
                        "  --assoc-weight LOG_NEW LOG_CLUTTER LOG_MISS: only with --assoc; a detection that starts a landmark adds LOG_NEW to its\n"
                        "              particle's log-likelihood, a dropped one LOG_CLUTTER, a landmark in view that took none (--prune) LOG_MISS;\n"
                        "              each finite and <= 0\n"
                        "  --pole-radius R [TOL]: only with --detect; a detection is the centre of the circle of radius R fitted to its segment,\n"
                        "              and segments more spread out than that circle (by more than TOL, default 0) are dropped\n"
                        "  --range-noise RANGE_VAR BEARING_VAR [LATERAL_VAR]: only with --detect and --assoc or --known-map, not with --meas-cov; every detection\n"
                        "              carries its own covariance (RANGE_VAR along its beam, BEARING_VAR r^2 + LATERAL_VAR across) and is gated under it\n"
                        "  --known-miss LOG_MISS VIEW_RANGE [--known-miss-fov EDGE] [--known-miss-sight BINS MARGIN]: only with --known-map; a map\n"
                        "      landmark within VIEW_RANGE of a pose that no detection matched costs LOG_MISS, unless outside the arc or hidden\n"
                        "  --known-reseed FRACTION [EVERY]: only with --known-map; behind every EVERY-th observing frame FRACTION of the particles\n"
                        "              becomes pose proposals from the frame's detections and the map (slam_pf_known_map_reseed)\n"
                        "  --known-reseed-pairs FRACTION TOL MIN_SEP [EVERY]: only with --known-map, not with --known-reseed; the same from PAIRS of\n"
                        "              detections at least MIN_SEP apart on two landmarks as far apart within TOL (slam_pf_known_map_reseed_pairs)\n"
                        "  --known-map FILE GATE MAP_VAR [LOG_CLUTTER]: localise in the landmark map of FILE (\"x,y\" lines, as --landmarks-out writes\n"
                        "              them; P = MAP_VAR * I each): every frame associates its detections (--detect) with that one map within GATE and\n"
                        "              weighs with the result, LOG_CLUTTER <= 0 per unmatched detection — with --range-noise under each detection's own\n"
                        "              covariance; one GPU, not with --landmarks or --meas-cov\n"
                        "  --spread-out FILE: one line per frame to FILE: frame, the covariance of the population over (x, y, sin dtheta) about its\n"
                        "              mean (xx, xy, yy, xs, ys, ss) and the length of the mean heading vector, %%.9g each; a small spread says the\n"
                        "              particles agree, not that they are right\n"
                        "  --modes-out FILE CELL HBINS M: one line per frame to FILE: frame, the number of modes, the number of occupied cells, then\n"
                        "              x y theta mass per mode of the population (slam_pf_modes: cells of CELL metres, HBINS heading bins — 1 or\n"
                        "              4 .. 64 —, at most M <= 8 modes, heaviest first), %%.9g each; one GPU, not with --gpus N > 1 or --transport\n", argv[0]);
        return 2;
    }
    if (run.use_meas_cov) {   /* the conditions of slam_pf_meas_cov_set: finite, qxx > 0, qyy > 0, float determinant > 0 */
        const float *q = run.meas_cov;
        const float xx = q[0] * q[2], xy = q[1] * q[1];
        if (!(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]) && q[0] > 0.0f && q[2] > 0.0f && xx - xy > 0.0f)) {
            fprintf(stderr, "--meas-cov %g %g %g: the values must be finite with QXX > 0, QYY > 0 and QXX * QYY - QXY * QXY > 0\n",
                    (double)q[0], (double)q[1], (double)q[2]);
            return 2;
        }
    }
    if (run.known_map) {
        FILE *km = fopen(run.known_map, "r");
        if (!km) { perror(run.known_map); return 2; }
        float *xy = (float *)malloc(sizeof(float) * 2 * SLAM_MAX_OBS);
        float px, py;
        int cnt = 0, got;
        while (xy && (got = fscanf(km, "%f,%f", &px, &py)) == 2 && cnt < SLAM_MAX_OBS) { xy[2 * cnt] = px; xy[2 * cnt + 1] = py; ++cnt; }
        const int clean = xy && feof(km);
        fclose(km);
        if (!clean || cnt < 1) {
            fprintf(stderr, "--known-map %s: expected 1 .. %d lines \"x,y\"\n", run.known_map, (int)SLAM_MAX_OBS);
            free(xy);
            return 2;
        }
        run.known_n = cnt;
        run.known_rows = (float *)calloc(5 * (size_t)cnt, sizeof(float));
        if (!run.known_rows) { free(xy); return 1; }
        for (int l = 0; l < cnt; ++l) {
            run.known_rows[l] = xy[2 * l];
            run.known_rows[cnt + l] = xy[2 * l + 1];
            run.known_rows[2 * cnt + l] = run.known_var;
            run.known_rows[4 * cnt + l] = run.known_var;
        }
        free(xy);
        if (!run.use_detect) fprintf(stderr, "--known-map without --detect: no frame has detections, the map is not used\n");
    }
    /* opened here: a rank that failed on it alone would leave the others waiting in their first collective */
    if (run.spread_out && !(run.spread = fopen(run.spread_out, "w"))) { perror(run.spread_out); free(run.known_rows); return 2; }
    if (run.modes_out && !(run.modes = fopen(run.modes_out, "w"))) { perror(run.modes_out); free(run.known_rows); return 2; }
    run.dataset = pos[0];
    run.frames = atoi(pos[1]);
    run.beams = atoi(pos[2]);
    run.map_out = pos[3];
    run.particles_total = atoi(pos[4]);
    if (npos > 5) run.seed = strtoull(pos[5], NULL, 10);
    if (npos > 6 && !strcmp(pos[6], "best")) run.use_mean = 0;
    if (run.particles_total <= 0 || run.particles_total % run.world) {
        fprintf(stderr, "particles must be a positive multiple of the number of GPUs\n");
        return 2;
    }
    if (run.same_device && !use_local && run.world > 1) {
        fprintf(stderr, "--same-device needs --transport local (RCCL refuses two ranks on one GPU)\n");
        return 2;
    }
    run.use_rccl = transport_given && !use_local;   /* "--gpus 1 --transport rccl": the sharded path on a one-rank group */
    if (use_local) {
        if (slam_local_group_create(run.world, &run.group) != SLAM_OK) return 1;
    } else if (run.world > 1 || run.use_rccl) {
        if (slam_comm_unique_id(run.comm_id) != SLAM_OK) {
            fprintf(stderr, "slam_comm_unique_id failed\n");
            return 1;
        }
    }

    rank_t ranks[16];
    pthread_t th[16];
    for (int r = 0; r < run.world; ++r) { ranks[r].run = &run; ranks[r].rank = r; ranks[r].rc = 1; }
    if (run.world == 1) {
        rank_main(&ranks[0]);
    } else {
        for (int r = 0; r < run.world; ++r)
            if (pthread_create(&th[r], NULL, rank_main, &ranks[r]) != 0) {
                /* the ranks already running would wait for this one in their first collective: end the whole program */
                fprintf(stderr, "pthread_create failed for rank %d\n", r);
                exit(1);
            }
        for (int r = 0; r < run.world; ++r) pthread_join(th[r], NULL);
    }
    int rc = 0;
    for (int r = 0; r < run.world; ++r) rc |= ranks[r].rc;
    slam_local_group_destroy(run.group);
    free(run.known_rows);
    if (run.spread && fclose(run.spread) != 0) { perror(run.spread_out); rc |= 1; }
    if (run.modes && fclose(run.modes) != 0) { perror(run.modes_out); rc |= 1; }
    return rc;
}
