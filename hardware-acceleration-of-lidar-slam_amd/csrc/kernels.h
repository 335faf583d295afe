// kernels.h — launchers of the gfx950 kernels, one section per kernel file in the Makefile's order; called by the C-ABI layer
// (engine.hip and engine_match / engine_ekf / engine_assoc / engine_evidence / engine_merge / engine_resample.hip by stage), the particle-filter session (the pf_session*.hip units) and the mapper (mapper.hip).
// Every launcher enqueues on `stream` and returns the hipError_t of the launch; none synchronises.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/slam_hip.h"

namespace slam {

// Optional timing of ONE kernel: when non-null, `start` is recorded immediately before and `stop`
// immediately after that kernel's launch on the same stream.
struct EventPair {
    hipEvent_t start = nullptr, stop = nullptr;
};

// ---- score_kernels.hip (reference: Subsystem_1/main.c:381-596)
struct ScoreGrid {
    const float* edt;   // [rows][ld]
    int rows, cols, ld;
    float ipix;         // 1 / pixel, computed on the host with one float division (main.c:383)
    float min_x, min_y;
    // Optional packed copy of the same grid for the many-pose scorers (launch_edt_pack): one BYTE per cell, stored in
    // vertical strips of 16 columns — cell (ix, iy) at (ix >> 4) * strip_bytes + iy * 16 + (ix & 15) — so that a 128-byte
    // line holds a 16 x 8 patch of cells, and a 256-entry table that turns a byte back into the cell's float, bit for bit.
    const uint8_t* packed = nullptr;
    const float* table = nullptr;
    int strip_bytes = 0;   // 16 * (rows rounded up to 8)
};
// The capped EDT (main.c:223-269, Appendix A.4) holds few distinct values: 0 on an occupied cell, sqrtf(d2) of a small
// integer d2 below the cap, and the cap itself.  launch_edt_pack writes code(cell) = d2 (255: the grid's largest value) into
// `packed`, table[code] = the float it stands for, and flag[1] = 1 if some cell of the rows x cols rectangle is not table[its
// code] bit for bit (a grid that did not come from the EDT kernels, or a cap above 16.0 cells with two different values of
// 16.0 and more: at cap 16.0 the largest distance below the cap is sqrtf(250) — 251 .. 255 are no sums of two squares — and
// 16.0 itself is the largest value): the caller then keeps the float grid.  flag: two device words {largest value's bits
// (scratch), bad}, zeroed by the launcher.
size_t edt_packed_bytes(int rows, int cols);
hipError_t launch_edt_pack(hipStream_t stream, const float* edt, int ld, int rows, int cols, uint8_t* packed, float* table,
                           uint32_t* flag);
// Pose-count threshold below which the scorers' 4-lanes-per-pose form wins (measured on MI355X, 360 beams, pipelined kernels of
// round 2: 64k poses 28.5 vs 30.1 us; 128k poses 55.4 vs 53.2 us; 256k poses 109 vs 104 us).
constexpr int kQuadMaxPoses = 131072;
// ... and below which one wavefront per pose wins over the quad form (360 / 1079 beams: 2k poses 6.1 vs 7.9 us / 18.3 vs
// 24.4 us; 4k poses 9.2 vs 8.0 us / 27.8 vs 24.6 us; 8k poses 14.9 vs 8.0 us / 44.1 vs 25.1 us).  The quad form is flat
// up to 8k poses: there its time is the chain of beam steps, not the work.
constexpr int kWaveMaxPoses = 3072;
hipError_t launch_score_poses(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                              const float* x, const float* y, const float* th_or_ct, const float* st_or_null,
                              int nposes, float* score, int32_t* count, const EventPair* ev = nullptr);
// motion sample fused in front of the score: pose' = motion(src[anc]), written to dst and scored
// A launch_free_list (paged_kernels.hip: the free list of a paged session, its arguments below) that travels in workgroups of its
// own behind those of a motion + score launch: neither needs anything from the other (free_list_body.h).
struct FreeListRider {
    const uint32_t* stamp = nullptr;   // nullptr: no rider
    int npages = 0;
    uint32_t live = 0;
    int32_t* freelist = nullptr;
    int32_t* pool_state = nullptr;
    int32_t* h_short = nullptr;
    int first_block = 0, nblocks = 0;   // filled in by the launcher
};
struct MotionIO {
    const float *sx, *sy, *sth;
    const int32_t* anc;
    float *x, *y, *th;
    FreeListRider rider;
};
// rider (optional): *rode says whether the launch took it along (the one-wavefront-per-pose form of small batches does not:
// the caller then launches the list by itself)
hipError_t launch_motion_score(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                               const MotionIO& io, int nposes, int64_t first_id, const float dp[3], const float sigma[3],
                               uint64_t seed, uint32_t frame, float* score, int32_t* count,
                               const EventPair* ev = nullptr, bool* rode = nullptr);
int free_list_blocks(int npages);
hipError_t launch_pose_hits(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                            const float* pose_xycs /*4 floats on device*/, float* hits, int32_t* count);

// The reference's 27-candidate lattice in one launch (FastMatch, main.c:440-573): candidate c gets one
// wavefront; score[c], count[c] and, in merged_hits, exactly what the reference leaves in its shared
// bestHits[] scratch after the sweep — entry j holds the hit of the LAST candidate (in evaluation
// order) that had more than j in-bounds beams (main.c:515 overwrites the prefix for every candidate).
// work: device scratch of 27*nbeams floats.  out layout: score[27] | count[27] (int) | maxcount (int) | merged[nbeams]
// d_nbeams (optional): the beam count lives on the device (<= nbeams, which then is the capacity / row stride).
// persist (optional): device mirror of the caller's persistent hit scratch, updated like the host copy.
// host_out / host_flag / seq (optional): also deliver `out` to mapped pinned host memory and release `seq`.
hipError_t launch_lattice(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                          const int32_t* d_nbeams, const float* cand_xycs /* X[27] Y[27] CT[27] ST[27] */, float* work,
                          float* out, float* persist, float* host_out, uint32_t* host_flag, uint32_t seq);
// FastMatch on g1 followed by FastMatch2 on g2 around its winner, THREE launches and no host in between (engine_match.hip:
// slam_engine_fastmatch_pair): the first lattice from cand1 as above; the second lattice's wavefronts work out the first call's
// winner themselves (strict '<' from +inf over out1's 27 scores, the first of equals; none: the middle candidate = the input
// pose) and lay their own candidate around it — x, y = the winner's -/+ pair_in[18], heading (cos, sin) = pair_in[3 a + b],
// pair_in[9 + 3 a + b] for the winner's heading a and the candidate's b —; one merge for both calls: the persistent hit scratch
// as the two calls one after the other leave it (entry j: the second call's where it has one, else the first call's), scores
// and counts of both calls to the host (host_out1: 54 words; host_out2: scores, counts, the second call's maxcount), the flag.
hipError_t launch_lattice_pair(hipStream_t stream, const ScoreGrid& g1, const ScoreGrid& g2, const float* bx, const float* by, int nbeams,
                               const int32_t* d_nbeams, const float* cand1, const float* pair_in, float* work1, float* work2, float* out1,
                               float* out2, float* persist, float* host_out1, float* host_out2, uint32_t* host_flag, uint32_t seq);

// ---- refine_kernels.hip (DESIGN.md §7 "Refinement"; no reference counterpart: FastMatch's lattice around every pose)
// `sweeps` sweeps of the 3 x 3 x 3 lattice (steps step_xy on x and y, step_theta on the heading; headings through det_sincosf)
// around each of nposes poses, the centre as incumbent; x / y / th are read and overwritten with the final pose, score / count
// are those of that pose as launch_score_poses gives them.  Uses g.packed when present, at any pose count.
hipError_t launch_refine_poses(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams, float* x, float* y,
                               float* th, int nposes, float step_xy, float step_theta, int sweeps, float* score, int32_t* count,
                               const EventPair* ev = nullptr);
// ... around pose' = motion(src[anc]) (launch_motion_sample's bits); io.x / io.y / io.th receive the refined pose only
hipError_t launch_motion_refine(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams, const MotionIO& io,
                                int nposes, int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame,
                                float step_xy, float step_theta, int sweeps, float* score, int32_t* count,
                                const EventPair* ev = nullptr);

// ---- edt_kernels.hip (row A6; reference: main.c:223-269, main_accelerated.c:215-283)
enum { EDT_MAX_RADIUS = 32 };
hipError_t launch_edt(hipStream_t stream, const int32_t* occ, int ld, int rows, int cols, float cap, float* out,
                      const EventPair* ev = nullptr);

// ---- ekf_kernels.hip, front_kernels.hip, ekf_sparse_kernels.hip (rows A9-A10; no reference counterpart): motion sample and landmark update
hipError_t launch_motion_sample(hipStream_t stream, const float* sx, const float* sy, const float* sth,
                                const int32_t* anc, float* x, float* y, float* th, int n, int64_t first_id,
                                const float dp[3], const float sigma[3], uint64_t seed, uint32_t frame);

struct EkfArgs {
    const float* map_in;
    float* map_out;
    int64_t row_stride;    // floats between consecutive particles' rows
    int plane_stride;      // floats between the five planes inside a row (>= nlandmarks)
    int nlandmarks;
    const float *x, *y, *th;
    const int32_t* anc;
    int n;
    const float *obs_zx, *obs_zy;   // device, indexed by landmark, padded to an even length; zx NaN = not observed
    float meas_var;
    float* loglik;        // [n], always written
    float* loglik_user;   // optional second copy for the caller
    int xcd_chunk;        // set by the launcher: workgroups per XCD when the grid is renumbered XCD-contiguously, else 0
    // ---- split layout (cov != nullptr; split_kernels.hip): map_in / map_out hold the MEANS only — rows of two planes
    // (mu_x, mu_y) of plane_stride floats, row_stride floats apart — and the covariance planes (P_xx, P_xy, P_yy) exist once
    // per COVARIANCE CLASS: in the world-frame update the posterior covariance of a landmark depends on its prior covariance,
    // on q and on whether the frame observes it, never on the particle, so particles whose covariances were equal once stay
    // equal for ever and share one row cov[class].  The update reads it (cov_update_body rewrites it afterwards, once per
    // class), hands the class of the source particle on to its offspring and marks it as still in use.
    const float* cov = nullptr;       // [classes][3][plane_stride]
    int64_t cov_stride = 0;           // floats between the rows of two classes
    const float* covx = nullptr;      // [classes][2][plane_stride]: 1 / det (P + q I) and 0.5 log det (P + q I) of the same covariances
    int64_t covx_stride = 0;          //   (ekf_math.h: ekf_det_terms), kept up to date by whoever writes cov
    const int32_t* cls_in = nullptr;  // class of every source particle
    int32_t* cls_out = nullptr;       // class of every particle of this frame
    uint32_t* cstamp = nullptr;       // [classes]: stamp_now = "a particle of this frame belongs to the class"
    uint32_t stamp_now = 0;
    // Sharded sessions, split layout: a frame's update in two launches.  Source rows below n are this rank's own particles;
    // rows from n on are the staging tail, filled by the exchange of the frame.  group_filter 1: only the groups (the particles
    // of one wavefront) whose sources are ALL local — they need nothing from the exchange and go out with the score, in the
    // fused front launch, before the host has even looked at the exchange plan; 2: only the other groups, behind the unpack.
    // 0: every group.
    int group_filter = 0;
    // Survivor rows (launch_ekf_materialise): the mean rows of a frame whose front launch wrote none, from the inputs that frame
    // started from.  survivor != nullptr: only particles i with survivor[i] == survivor_stamp (the ones the frame's resample
    // kept) get their row; a wavefront without one leaves before it loads anything else.  nullptr: every particle.
    const uint32_t* survivor = nullptr;
    uint32_t survivor_stamp = 0;
};
// the split layout's part of EkfArgs, as the session hands it to the engine's stage functions
struct SplitIO {
    int group_filter;          // EkfArgs::group_filter
    const int32_t* map_anc;    // the gather index of the MAPS when it is not the scorer's pose index (sharded: poses come out of
                               // the all-gathered array of every rank, maps out of the local rows + staging tail); nullptr: the same
    const float* cov;
    int64_t cov_stride;
    const float* covx;
    int64_t covx_stride;
    const int32_t* cls_in;
    int32_t* cls_out;
    uint32_t* cstamp;
    uint32_t stamp_now;
};
// group_size: 0 = one wavefront per particle; 2 / 4 / 8 = the grouped out-of-place form (that many neighbouring particles
// per wavefront share their source rows in registers) — a speed choice only, every form gives the same bits
hipError_t launch_ekf_update(hipStream_t stream, const EkfArgs& a, const EventPair* ev = nullptr, int group_size = 0);
// split layout: the MEAN ROWS of launch_ekf_update alone, bit for bit — no log-likelihood, no class, no stamp is written; reads
// the stored poses a.x / a.y / a.th; optionally for the survivors only (EkfArgs::survivor).  group_size as above.
hipError_t launch_ekf_materialise(hipStream_t stream, const EkfArgs& a, const EventPair* ev, int group_size);
// The same update with a full 2x2 measurement covariance Q in the sensor frame (ekf_aniso_math.h, ekf_aniso_lane.h; rows
// only: the posterior covariance then depends on the particle's heading).  Q and its float32 determinant:
struct EkfAnisoCov {
    float qxx, qxy, qyy, detq;
};
// detq = qxx * qyy - qxy * qxy: two products and one subtraction, each rounded to float32 (-ffp-contract=off)
inline EkfAnisoCov ekf_aniso_cov(const float meas_cov[3])
{
    EkfAnisoCov q{ meas_cov[0], meas_cov[1], meas_cov[2], 0.0f };
    const float xx = q.qxx * q.qyy, xy = q.qxy * q.qxy;
    q.detq = xx - xy;
    return q;
}
// every value finite, qxx > 0, qyy > 0 and the float32 determinant > 0 (NaN fails every comparison)
__host__ __device__ inline bool ekf_aniso_cov_ok(const EkfAnisoCov& q)
{
    const float big = 3.402823466e+38f;
    return q.qxx > 0.0f && q.qyy > 0.0f && q.detq > 0.0f && q.qxx <= big && q.qyy <= big && q.qxy >= -big && q.qxy <= big;
}
// A per-particle table a landmark update reads its observations through: z of landmark l of particle i = det[assoc[i][l]]
// (data association, assoc_kernels.hip below, makes it)
struct EkfAssocTable {
    const uint8_t* assoc;
    int assoc_stride;
    const float *det_zx, *det_zy;
    int ndet;
};
// The one-wavefront-per-particle form of launch_ekf_update (which delegates to it) under either noise and either source of
// observations: out of place (through a.anc, landmarks without an observation copied) or in place (a.map_in == a.map_out: only
// landmarks with one touched); a.cov must be null. q == nullptr: noise a.meas_var * I, else R_w(theta_i) of *q (a.meas_var is not read; ekf_aniso_cov_ok(*q)).
// tab == nullptr: observations a.obs_zx / a.obs_zy, else through *tab (a.obs_zx / a.obs_zy are not read).
hipError_t launch_ekf_rows(hipStream_t stream, const EkfArgs& a, const EkfAnisoCov* q, const EkfAssocTable* tab, const EventPair* ev = nullptr);
// A measurement covariance PER DETECTION (specification: tests/_assoc_detcov_spec.py): Q_k = {qxx[k], qxy[k], qyy[k]} in the
// sensor frame beside detection k of an EkfAssocTable / of AssocArgs, every one by the rule of ekf_aniso_cov_ok (whoever hands
// them over has checked that, or made them so); det Q_k is formed from them where it is needed, never handed in
struct DetCovArgs {
    const float *qxx, *qxy, *qyy;   // [ndet]
    int ndet;
};
// ... the row update through *tab with R_w(theta_i, k) of the detection each landmark of particle i takes (a.meas_var is not read)
hipError_t launch_ekf_rows_detcov(hipStream_t stream, const EkfArgs& a, const DetCovArgs& q, const EkfAssocTable& tab, const EventPair* ev = nullptr);
// ---- assoc_kernels.hip: data association (specification: tests/_assoc_spec.py).  The detections of a frame
// are sensor-frame points WITHOUT identity; every particle decides for itself which of its landmarks each one belongs to and
// which ones start a new landmark.  Rows only: the table is per particle, so "which landmarks a frame observes" is too.
struct AssocArgs {
    const float* map;      // rows as in EkfArgs (read only)
    int64_t row_stride;
    int plane_stride;
    int nlandmarks;        // <= SLAM_MAX_OBS
    const float *x, *y, *th;
    const int32_t* anc;    // particle i reads row anc[i] (nullptr: i)
    int n;
    const float *det_zx, *det_zy;   // [ndet] finite sensor-frame points
    int ndet;                       // <= SLAM_MAX_DETECTIONS
    float meas_var, gate, new_gate;
    uint8_t* assoc;        // [n][assoc_stride]: entry l = the detection landmark l takes, SLAM_ASSOC_NONE = none
    int assoc_stride;      // >= nlandmarks; the columns from nlandmarks on are written SLAM_ASSOC_NONE
    int32_t* stats;        // [n][3] matched, created, dropped; may be nullptr
    int xcd_chunk;         // set by the launcher
};
// one wavefront per particle; create: unmatched detections far from every seen landmark take the unseen slots.  The noise every
// particle gates, matches and creates under, at most one of q and dq: neither — a.meas_var * I; q — a full 2x2 sensor-frame
// covariance, S = P + R_w(theta_i) (specification: tests/_assoc_aniso_spec.py; ekf_aniso_cov_ok(*q) is checked); dq — a Q_k per
// detection, S = P + R_w(theta_i, k) (dq->ndet == a.ndet).  Under q or dq a.meas_var is not read
hipError_t launch_associate(hipStream_t stream, const AssocArgs& a, const EkfAnisoCov* q, const DetCovArgs* dq, bool create,
                            const EventPair* ev = nullptr);
// ---- localise_kernels.hip: localisation in a known landmark map (specification: tests/_localise_spec.py).
// ONE map every particle shares, never changed: what depends on a covariance is prepared once per map, and the stage associates
// the frame's detections per particle (create = 0) and leaves the matched pairs' log-likelihood.  No rows.
struct KnownMapArgs {
    const float* map;      // [5][plane_stride]: mx, my, P_xx, P_xy, P_yy; P_xx < 0: the slot holds no landmark
    int plane_stride;
    int nlandmarks;        // 1 .. SLAM_MAX_OBS
    float meas_var;
    float* prep;           // [6][plane_stride]: mx (NaN: no landmark), my, i00, i01, i11, hl
};
// one thread per slot of the plane stride
hipError_t launch_known_map_prepare(hipStream_t stream, const KnownMapArgs& a, const EventPair* ev = nullptr);
struct LocaliseArgs {
    const float* map;      // the prepared map [6][plane_stride] — under a DetCovArgs: the map as it was given [5][plane_stride]
    int plane_stride;
    int nlandmarks;        // 1 .. SLAM_MAX_OBS
    const float *x, *y, *th;
    int n;
    const float *det_zx, *det_zy;   // [ndet] finite sensor-frame points
    int ndet;                       // <= SLAM_MAX_DETECTIONS
    float gate;
    uint8_t* assoc;        // [n][assoc_stride] as AssocArgs::assoc; nullptr: no table is written
    int assoc_stride;
    int32_t* stats;        // [n][3] matched, 0, dropped
    float* loglik;         // [n]
};
// one wavefront per particle at a time, persistent workgroups; the map staged in LDS where it fits.  q == nullptr: a.map is the
// prepared map; else S = P + R_w(theta_i, k), Q_k per detection (specification: tests/_localise_detcov_spec.py; q->ndet == a.ndet):
// nothing can be prepared, a.map is the RAW map (KnownMapArgs::map) and S^-1 is formed per (landmark, detection) pair.
// v != nullptr: the MISS form of either (specification: tests/_localise_miss_spec.py) — the same launch also counts, per particle,
// the landmarks the map predicts in view that no detection matched, under the evidence stage's own predicate; loglik, stats and the
// table are what the launch without v writes, bit for bit
struct LocMissArgs {
    float range2;          // view_range * view_range, one float32 product made on the host
    int fov;               // 0: the whole circle (lo, hi are not read)
    float lo, hi;          // as FovArgs
    const float* table;    // [bins] a sight table (launch_sight_table); nullptr: no line of sight (bins = 0 then)
    int bins;
    float margin;          // as SightArgs
    int32_t* missed;       // [n] seen, matched by no detection, within view_range, in the arc, not hidden
    int32_t* spared;       // [n] ... in the arc and hidden; may be nullptr
    int32_t* outside;      // [n] ... outside the arc; may be nullptr
};
hipError_t launch_localise(hipStream_t stream, const LocaliseArgs& a, const DetCovArgs* q, const LocMissArgs* v = nullptr,
                           const EventPair* ev = nullptr);
// ---- reseed_kernels.hip: reseeding the cloud from what the lidar sees (specification: tests/_reseed_spec.py).
// A chosen fraction of the slots becomes pose proposals at which one detection coincides with one landmark of the known map; the
// rest take the pending resample.
struct ReseedArgs {
    const float* map;      // the map as it was given [5][plane_stride] (KnownMapArgs::map); P_xx < 0: the slot holds no landmark
    int plane_stride;
    int nlandmarks;        // >= 1, <= plane_stride
    const float *x_in, *y_in, *th_in;
    const int32_t* anc;    // a slot that is not replaced copies the pose of anc[i] (nullptr: i, and out may be in)
    float *x_out, *y_out, *th_out;
    int n;
    const float *det_zx, *det_zy;   // [ndet] sensor-frame points
    int ndet;                       // 1 .. SLAM_MAX_DETECTIONS
    uint64_t first_id;     // global id of slot 0
    uint32_t key0, key1, frame;
    uint64_t thr;          // floor(fraction * 2^32), 1 .. 2^32: slot i is chosen iff its first Philox word is below it
    uint8_t* flag;         // [n] 1 replaced, 2 chosen but its landmark slot is empty, 0 otherwise; may be nullptr
    unsigned int* acc;     // {replaced, chosen but not replaced, ticket}: zero on entry, left zero
    int32_t* out;          // [2] the two counts
    int32_t* h_out;        // the same in mapped host memory behind *h_seq = seq; may be nullptr
    uint32_t* h_seq;
    uint32_t seq;
};
// one thread per slot; the counts are exact (one atomic per workgroup and count, handed over by the last workgroup to arrive)
hipError_t launch_pose_reseed(hipStream_t stream, const ReseedArgs& a, const EventPair* ev = nullptr);
// ---- reseed_pair_kernels.hip: reseeding from detection PAIRS (specification: tests/_reseed_pair_spec.py).  A
// chosen fraction of the slots becomes pose proposals at which two detections coincide with two landmarks of the known map — the
// first landmark and both detections drawn, the second landmark searched for by the wavefront; the rest take the pending resample.
struct ReseedPairArgs {
    const float* map;      // the map as it was given [5][plane_stride] (KnownMapArgs::map); P_xx < 0: the slot holds no landmark
    int plane_stride;
    int nlandmarks;        // >= 2, <= plane_stride
    const float *x_in, *y_in, *th_in;
    const int32_t* anc;    // a slot that is not replaced copies the pose of anc[i] (nullptr: i, and out may be in)
    float *x_out, *y_out, *th_out;
    int n;
    const float *det_zx, *det_zy;   // [ndet] sensor-frame points
    int ndet;                       // 2 .. SLAM_MAX_DETECTIONS
    uint64_t first_id;     // global id of slot 0
    uint32_t key0, key1, frame;
    uint64_t thr;          // floor(fraction * 2^32), 1 .. 2^32: slot i is chosen iff its first Philox word (stream 2) is below it
    float tol;             // >= 0: a landmark is a partner if its distance from j1 is the detections' distance within tol
    float min_sep2;        // (min_sep * min_sep, rounded once; min_sep > tol): detections closer than that make no pair
    uint8_t* flag;         // [n] 1 replaced, 2 slot j1 empty, 3 detections too close, 4 no partner, 0 not chosen; may be nullptr
    unsigned int* acc;     // {replaced, j1 empty, too close, no partner, ticket}: zero on entry, left zero
    int32_t* out;          // [4] the four counts
    int32_t* h_out;        // the same in mapped host memory behind *h_seq = seq; may be nullptr
    uint32_t* h_seq;
    uint32_t seq;
};
// one thread per slot, the search by its wavefront; the counts are exact (one atomic per workgroup and count, handed over by the
// last workgroup to arrive)
hipError_t launch_pose_reseed_pairs(hipStream_t stream, const ReseedPairArgs& a, const EventPair* ev = nullptr);
// ---- evidence_kernels.hip: landmark existence evidence (specification: tests/_evidence_spec.py).  One byte
// c in [0, cmax] per (particle, landmark slot) beside the rows; behind the update of a frame a matched landmark gains `hit`, a
// visible unmatched one loses `miss`, and one that cannot pay is pruned: its slot gets the bits of a slot that was never used.
struct EvidenceArgs {
    float* map;            // rows as in EkfArgs, AFTER the frame's update: read, and written where a landmark is pruned
    int64_t row_stride;
    int plane_stride;
    int nlandmarks;        // <= SLAM_MAX_OBS
    const float *x, *y;    // the poses the update used
    const int32_t* anc;    // particle i reads evidence row anc[i] (nullptr: i; the MAP row is always i)
    int n;
    const uint8_t* assoc;  // [n][assoc_stride] the frame's table
    int assoc_stride;      // >= nlandmarks
    int ndet;              // K: a table byte < K is a hit
    const uint8_t* ev_in;  // [rows][ev_stride]
    uint8_t* ev_out;       // [n][ev_stride]; == ev_in: in place (anc must be nullptr), the padding columns are left alone — else written 0
    int ev_stride;         // >= nlandmarks
    int hit, miss, cmax;   // 1 .. 255
    float range2;          // view_range * view_range, one float32 product made on the host
    int32_t* stats;        // [n][2] pruned, seen after pruning; may be nullptr
    int32_t* missed;       // [n] landmarks the stage scored as a miss (lowered or pruned), in whichever form runs; may be nullptr
    int xcd_chunk;         // set by the launcher
};
// the two rules that spare a landmark due a miss (seen, not hit, within view_range); each is a switch of the one stage.
// LINE OF SIGHT (specification: tests/_sight_spec.py): hidden behind what the scan hit in its direction
struct SightArgs {
    const float* th;       // [n] the headings the update used (beside EvidenceArgs::x / y); read under either rule
    const float* table;    // [bins] a sight table (launch_sight_table)
    int bins;
    float margin;          // > 0: hidden = the nearest return of the landmark's bin and its two neighbours < (r - margin)^2
    int32_t* spared;       // [n] landmarks due a miss and hidden; may be nullptr
};
// FIELD OF VIEW (specification: tests/_fov_spec.py): its sensor-frame direction (the diamond angle p) outside the arc
struct FovArgs {
    float lo, hi;          // in [0, 4]; lo <= hi: in view = lo <= p <= hi; lo > hi: p >= lo || p <= hi (the arc through p = 4 = 0)
    int32_t* outside;      // [n] landmarks due a miss and outside the arc; may be nullptr
};
bool fov_bounds_ok(float lo, float hi);
// one wavefront per particle; byte traffic as dwords when every row of the three byte arrays starts on a dword, else as bytes.
// miss_now = due & in view & ~hidden.  sg == fv == nullptr: everything is in view, nothing hidden.  sg alone: line of sight.
// fv (sg with it, for th): the arc test first; sg->table == nullptr then: without line of sight (nothing is hidden; sg->bins and
// sg->margin are not read, sg->spared is written 0).  One grid, the same lanes and byte paths in every form
hipError_t launch_landmark_evidence(hipStream_t stream, const EvidenceArgs& a, const SightArgs* sg, const FovArgs* fv,
                                    const EventPair* ev = nullptr);
struct EvidenceInitArgs {
    const float* map;      // [nrows] rows as above (read only)
    int64_t row_stride;
    int plane_stride;
    int nlandmarks;
    int nrows;
    uint8_t* ev;           // [nrows][ev_stride] <- seen ? value : 0, the padding columns 0
    int ev_stride;
    int value;             // 0 .. 255
    int xcd_chunk;         // set by the launcher
};
hipError_t launch_evidence_init(hipStream_t stream, const EvidenceInitArgs& a, const EventPair* ev = nullptr);
// a frame without a landmark update: the evidence follows its particles, out[i] = in[anc[i]] (whole rows of `stride` bytes)
hipError_t launch_evidence_gather(hipStream_t stream, const uint8_t* in, uint8_t* out, int stride, const int32_t* anc, int n);
// ---- sight_kernels.hip: the table behind the evidence stage's line of sight (specification: tests/_sight_spec.py; DESIGN.md
// section 7).  The SIGHT TABLE of a scan: per direction bin (the diamond angle of a sensor-frame point in `bins` equal steps) the smallest
// squared range of the scan's points in it, +inf: none.  A landmark behind what the table holds in its direction is hidden.
constexpr int kSightMinBins = 32, kSightMaxBins = 1024;
bool sight_bins_ok(int bins);   // a power of two in kSightMinBins .. kSightMaxBins
// one workgroup over the scan; out: kSightMaxBins floats, the first `bins` the table, +inf behind them
hipError_t launch_sight_table(hipStream_t stream, const float* bx, const float* by, int nbeams, int bins, float* out, const EventPair* ev = nullptr);
// ---- merge_kernels.hip: merging duplicate landmarks (specification: tests/_merge_spec.py).  Behind the
// frame's associating update (and its evidence stage), in place: a seen landmark the frame's table does not name (free) that lies
// within merge_gate — the Mahalanobis term of mu_l - mu_w under P_l + P_w — of a landmark it names (an anchor) is fused into it.
struct MergeArgs {
    float* map;            // rows as in EkfArgs, AFTER the frame's update: read, and written where a pair is merged
    int64_t row_stride;
    int plane_stride;
    int nlandmarks;        // <= SLAM_MAX_OBS
    int n;
    const uint8_t* assoc;  // [n][assoc_stride] the frame's table
    int assoc_stride;      // >= nlandmarks
    int ndet;              // K: a table byte < K names an anchor
    uint8_t* ev;           // [n][ev_stride] evidence bytes, in place; nullptr: without evidence (ev_stride and cmax are not read)
    int ev_stride;         // >= nlandmarks
    int cmax;              // 1 .. 255
    float gate;            // finite, > 0
    int32_t* stats;        // [n][3] merged, refused, seen after the stage; may be nullptr
    int xcd_chunk;         // set by the launcher
};
bool merge_args_ok(const MergeArgs& a);
// one wavefront per particle; the table's bytes as dwords when every row of it starts on a dword, else as bytes
hipError_t launch_landmark_merge(hipStream_t stream, const MergeArgs& a, const EventPair* ev = nullptr);
// ---- assoc_weight_kernels.hip: the weight of what the association leaves unexplained (specification:
// tests/_assoc_weight_spec.py).  Behind the frame's update, evidence stage and merge, in front of the weights:
// loglik[i] += created_i * log_new + dropped_i * log_clutter + missed_i * log_miss, every operation rounded once.
struct AssocWeightArgs {
    const int32_t* stats;   // [n][3] the association's matched, created, dropped
    const int32_t* missed;  // [n] EvidenceArgs::missed of the frame; nullptr: 0 (pruning off)
    int n;
    float log_new, log_clutter, log_miss;   // finite, <= 0
    float* loglik;          // [n] read and written
    float* terms;           // [n] the sum that was added; may be nullptr
};
bool assoc_weight_const_ok(float v);
// one thread per particle
hipError_t launch_assoc_weight(hipStream_t stream, const AssocWeightArgs& a, const EventPair* ev = nullptr);
// ---- detect_kernels.hip: the landmark detector (specification: tests/_detect_spec.py).  The scan's short,
// narrow, unoccluded runs of points between two range jumps become the frame's detections: their centroids, in scan order.
// fit (specification: tests/_detect_fit_spec.py): the runs that are no more spread out than a circle of the given radius, each
// as that circle's centre.
struct DetectArgs {
    const float *bx, *by;   // the scan, [nbeams] sensor-frame points in scan order
    int nbeams;             // 0 .. SLAM_MAX_BEAMS
    float jump2, guard2, width2, range2;   // the squares of slam_detect_params' lengths, one float32 product each, made on the host
    int min_points, max_points, wrap;      // 1 <= min_points <= max_points <= SLAM_DETECT_MAX_POINTS
    float* det;             // zx[SLAM_MAX_DETECTIONS] | zy[SLAM_MAX_DETECTIONS]: the first ndet by ascending start, then 0
    int32_t* stats;         // [4] segments, accepted, written (= ndet), rejected by the shape test (0 without fit); may be nullptr
    int32_t* h_out;         // mapped host memory {ndet, sequence}: plain stores, `seq` released last
    uint32_t seq;
    // behind everything the kernel without the fit reads:
    int fit;                // 0: the centroid; 1: the centre of a circle of squared radius rho2 through the segment
    float rho2, lim;        // radius * radius; rho2 + spread_tol * spread_tol: one float32 operation each, made on the host
};
// The detector's noise model (specification: tests/_detect_noise_spec.py): a detection (zx, zy) that passed its range test gets
// Q = a u u^T + b v v^T, u its line of sight, a = range_var, b = bearing_var * r2 + lateral_var; one whose r2 is 0 or whose Q
// fails ekf_aniso_cov_ok is no detection (counted in stats[4] of then six words, stats[5] = 0), in front of the cap at 64
struct DetectNoiseArgs {
    float range_var, bearing_var, lateral_var;
    float* cov;             // qxx[SLAM_MAX_DETECTIONS] | qxy[..] | qyy[..]: the first ndet, then 0
};
// one workgroup of 64 .. 1024 threads by the size of the scan; noise == nullptr: the kernels without the model, as they were
hipError_t launch_detect_scan(hipStream_t stream, const DetectArgs& a, const EventPair* ev = nullptr, const DetectNoiseArgs* noise = nullptr);
bool frame_front_fits(int n, int nlandmarks, int group_size);   // the shapes launch_frame_front takes
// motion sample + scan-match score AND the grouped out-of-place landmark update in ONE launch (single-GPU frames on rows): the
// gathers of the scorer run in the shadow of the update's row stores.  `a.x / a.y / a.th` are not read (the update works out
// its particles' motion samples itself, the same bits the scorer writes to io.x / io.y / io.th).  *launched = false: shapes
// that this kernel does not take; nothing was issued.
// obs_save (split layout only; nullptr: none): the launch writes NO mean row — everything else as ever, the same bits — and one
// more workgroup copies the observation table to obs_save [2][plane_stride] (zx | zy), for launch_ekf_materialise to start from.
// weights (optional): where the frame's log-weights and their block maxima go when ONE workgroup can both score and update
// its particles (frame_particle_kernel: a survivor-rows frame of the split layout, 8 particles per wavefront, four lanes per
// pose, one GPU, at most kMaxWeightBlocks workgroups of 64 particles); *weights->made says whether it did: then block_max
// holds ceil(n / 64) maxima and no weights' launch is wanted.  Every other frame: the launch as ever, *made = false.
constexpr int kMaxWeightBlocks = 2048;   // the block maxima a frame leaves at most, whichever launch makes them (logweight_scratch_floats)
struct FrontWeights {
    float gain;
    float* logw;
    float* block_max;
    const float* carry;                // as launch_logweight's
    const int32_t* prev_resampled;
    bool* made;
};
hipError_t launch_frame_front(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                              const MotionIO& io, int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed,
                              uint32_t frame, float* score, int32_t* count, const EkfArgs& a, int group_size,
                              const EventPair* ev, bool* launched, int* lanes_per_pose = nullptr, float* obs_save = nullptr,
                              const FrontWeights* weights = nullptr);
// In-place update of the OBSERVED landmarks only (frames that keep their population): the observation table is first
// compacted into a list in landmark order (ids, measurements, accumulator rounds; count[2] = {nobs, highest round} on the
// device, {nobs, L} optionally in mapped host memory), then one lane per observation gathers, updates and scatters.
constexpr int kObsListMaxLandmarks = 65536;   // the list form keeps a bitmap of the observed landmarks in LDS
// the list: ids ascending, measurements, accumulator rounds, {nobs, highest round}
struct ObsListView {
    const int32_t* id = nullptr;
    const float *zx = nullptr, *zy = nullptr;
    const int32_t* round = nullptr;
    const int32_t* count = nullptr;
};
struct ObsListOut {   // where launch_build_obs_list and launch_page_list leave it (id == nullptr: none wanted)
    int32_t* id = nullptr;
    float *zx = nullptr, *zy = nullptr;
    int32_t *round = nullptr, *count = nullptr;
};
hipError_t launch_build_obs_list(hipStream_t stream, const float* tzx, const float* tzy, int L, const ObsListOut& ol, int32_t* h_count);
hipError_t launch_ekf_sparse(hipStream_t stream, const EkfArgs& a, const ObsListView& ol, const EventPair* ev = nullptr);
// measurement support: rows of 5 x plane_stride floats copied with the update's access shape (slam_profile_copy_ceiling)
hipError_t launch_copy_rows(hipStream_t stream, const float* in, float* out, int n, int plane_stride);
// every float in the fast reciprocal's range, ekf_rcp_core against IEEE division
hipError_t launch_selftest_reciprocal(hipStream_t stream, unsigned long long* out /* [2], zeroed: mismatches, values checked */);

// ---- paged_kernels.hip: landmark maps as copy-on-write pages of kPageLandmarks landmarks (5 planes x 32 floats = 640 B)
constexpr int kPageLandmarks = 32;   // 16- and 8-landmark pages measured no faster: profiles/r03_page_sizes.md
// Where a page lies.  The pages of a session on joint pages are one array of [5][32] floats; the pages of a SPLIT session on
// pages hold the two planes of MEANS only ([2][32] floats, 256 bytes) and lie in the session's two mean buffers, which are
// not neighbours in the store: pages below `half_pages` in the first, the others `gap` floats further on.
struct PageGeom {
    int planes = 5;                          // planes per page (5: means + covariances; 2: means)
    int64_t half_pages = (int64_t)1 << 62;   // pages at or beyond this index lie `gap` floats further on
    int64_t gap = 0;
};
// A session's page pool as the launchers off the frame path take it (pf_session_store.hip: page_pool): by const reference to a
// launcher, by value to its kernel.  pt is ONE table (the session's current one unless the caller says otherwise).
struct PagePool {
    float* pool;           // [npages][geom.planes][32]
    PageGeom geom;
    int32_t* pt;           // [rows][nb]
    int nb;                // pages per particle
    int32_t* freelist;     // [npages]
    int npages;
    int32_t* pool_state;   // pool_state_words() int32, see below
    uint32_t* stamp;       // [npages]
    uint32_t stamp_now;    // the stamp of the last update: pages that carry it are in use
};
// ... and the covariance classes of a session on the split layout or on split pages (split_kernels.hip; class_store)
struct ClassStore {
    float* cov;           // [classes][3][Lp], see EkfArgs
    float* covx;          // [classes][2][Lp]
    int32_t* cls;         // [rows] class of every particle (the current buffer)
    int Lp;               // floats between the planes of a class row
    uint32_t* cstamp;     // [classes]
    uint32_t stamp_now;   // the stamp of the last update: classes that carry it are in use
    int32_t* live;        // the current list of classes in use ...
    int32_t* cnt;         // ... and its length, one of three rotating words (CovArgs); at the start of an epoch the first of them
};
struct PagedEkfArgs {
    PageGeom geom;
    // split session on pages (geom.planes == 2): the covariances come per class, as in EkfArgs
    const float* cov = nullptr;
    const float* covx = nullptr;
    int plane_stride = 0;             // floats between the planes of a class row (Lp)
    const int32_t* cls_in = nullptr;
    int32_t* cls_out = nullptr;
    uint32_t* cstamp = nullptr;
    uint32_t cstamp_now = 0;
    float* pool;             // [npages][planes][32]
    const int32_t* pt_in;    // [rows][nb] page tables of the ancestors
    int32_t* pt_out;         // [n][nb]    page tables of this frame's particles
    int nb;                  // pages per particle
    const int32_t* anc;      // source table of particle i (nullptr: i)
    int n, nlandmarks;
    const float *x, *y, *th;
    const float *obs_zx, *obs_zy;   // table form, NaN = not observed
    float meas_var;
    float* loglik;
    float* loglik_user;
    const int32_t *tpage, *tindex, *count;   // launch_page_list of the same table
    const int32_t* tmask;                    // ... bit s of tmask[t]: landmark s of touched page t is observed
    const int32_t* tbase;                    // ... tbase[t]: observations in the touched pages before t (tbase[T]: all)
    ObsListView ol;                          // the same observations as a list (the list form of the update)
    const int32_t* freelist;                 // particle i takes entries pool_state[base] + [i * T, (i + 1) * T)
    const int32_t* pool_state;               // written by launch_page_list of this frame
    uint32_t* stamp;                         // [npages]: every page a new table names gets stamp_now
    uint32_t stamp_now;
};
// pool_state (pool_state_words() int32 on the device): the free list's bookkeeping — how long it is, how much of it has
// been handed out, whether launch_free_list (to be called behind this launcher every frame) has to make a new one first
int pool_state_words();
// h_obs + votes (optional): the launch also takes SLAM_MAP_AUTO's sample — votes[2] (device): samples in a row with at most
// two sevenths / more than three eighths of the landmarks observed; h_obs (mapped host memory): {observed, L, seq, votes[0], votes[1]}
hipError_t launch_page_list(hipStream_t stream, const float* zx, const float* zy, int L, int nb, int32_t* tpage, int32_t* tindex,
                            int32_t* tmask, int32_t* tbase, int32_t* count, int n, int32_t* pool_state, int32_t* h_obs = nullptr,
                            uint32_t seq = 0, int32_t* votes = nullptr, int32_t* h_touched = nullptr,
                            const ObsListOut& ol = ObsListOut());
// the same sample as a launch of its own (one small workgroup), for sessions on rows
hipError_t launch_obs_count(hipStream_t stream, const float* zx, const float* zy, int L, int32_t* h_obs, uint32_t seq, int32_t* votes);
// form 0: every lane of a touched page runs the update arithmetic, one page after the other; form 1 (needs a.ol): the
// touched pages go through an LDS image, several at a time with all their loads in flight together, and the arithmetic
// runs once per observation, one lane each — the same bits.  touched_hint: pages to stage per pass (<= 0: a default)
hipError_t launch_ekf_paged(hipStream_t stream, const PagedEkfArgs& a, const EventPair* ev = nullptr, int form = 1,
                            int touched_hint = 0);
hipError_t launch_page_table_gather(hipStream_t stream, const int32_t* pt_in, int32_t* pt_out, int nb, const int32_t* anc, int n,
                                    uint32_t* stamp, uint32_t stamp_now);
// free list = pages whose stamp differs from `live`, the stamp of the last update (in no particular order); does
// nothing unless launch_page_list asked for it
// h_short (optional, mapped host memory): set to 1 when a list made anew turns out shorter than the reservation
hipError_t launch_free_list(hipStream_t stream, const uint32_t* stamp, int npages, uint32_t live, int32_t* freelist,
                            int32_t* pool_state, int32_t* h_short = nullptr);
// out[k] = anc[sel[k]] (anc == nullptr: sel[k])
hipError_t launch_compose_index(hipStream_t stream, const int32_t* sel, const int32_t* anc, int count, int32_t* out);
// rows -> pages page_base + j * nb + b behind identity tables; every other page of the pool goes on the free list
hipError_t launch_pages_from_rows(hipStream_t stream, const float* rows, int64_t row_stride, int plane_stride, int nlandmarks, int n,
                                  const PagePool& pp, int page_base = 0);
// pages of particle anc[i] (or i) -> row i of geom.planes planes
hipError_t launch_rows_from_pages(hipStream_t stream, const PagePool& pp, const int32_t* anc, int n, float* rows, int64_t row_stride,
                                  int plane_stride, int nlandmarks);
// the first nentries table entries name ONE shared page of landmarks "not seen yet" (page 0), the rest of the pool is free
hipError_t launch_pages_reset(hipStream_t stream, const PagePool& pp, int64_t nentries);
// split pages -> dense rows of 5 planes (means from the particle's pages of two planes, covariances from its class's rows)
hipError_t launch_rows_from_split_pages(hipStream_t stream, const PagePool& pp, const ClassStore& cs, const int32_t* idx, int count,
                                        float* rows, int64_t row_stride, int plane_stride, int nlandmarks);
// Sharded sessions: `want` pages for the rows about to be unpacked (pool_state then says where in the list they start and
// whether launch_free_list, to be called behind it, has to make a new list first), and the unpack itself: record p of
// `in` (pose + 5 x nlandmarks floats, as launch_migrate_pack writes them) -> table row n + p on fresh pages, stamped pp.stamp_now
hipError_t launch_pool_reserve(hipStream_t stream, int32_t* pool_state, int64_t want);
// ... for a session on SPLIT PAGES: record p -> its means on fresh pages of two planes behind table row n + p, its covariances (and
// their determinant terms, meas_var) as class cls_free[cls_first + p] of its own, appended to the list of classes in use
hipError_t launch_migrate_unpack_split_pages(hipStream_t stream, const float* in, int total, int n, float* pose, int64_t pose_ld,
                                             const PagePool& pp, const ClassStore& cs, int nlandmarks, float meas_var,
                                             const int32_t* cls_free, int cls_first);
hipError_t launch_migrate_unpack_paged(hipStream_t stream, const float* in, int total, int n, float* pose, int64_t pose_ld,
                                       const PagePool& pp, int nlandmarks);

// ---- split_kernels.hip: the covariance classes of the split layout (see EkfArgs)
// The posterior covariance of every class that is still in use, in place, once per class: P' = (I - W) P for an observed
// landmark seen before, q I for a first sighting, the prior without an observation — the values every particle of the class
// would have written into its own row (ekf_math.h: ekf_shared).  `live`: the classes that were in use after the previous
// frame, cnt[phase] of them; those that still are (cstamp == stamp_now) are updated and appended to the next list (cnt[(phase
// + 1) % 3]; cnt[(phase + 2) % 3] is zeroed for the frame after).  bound >= cnt[phase]: the launch's width (the host's stale
// knowledge is good enough: the list only shrinks).  h_live (mapped host memory): {cnt[phase], epoch}.
struct CovArgs {
    float* cov;
    int64_t cov_stride;
    float* covx;           // the determinant terms of the NEW covariances go here (EkfArgs::covx)
    int64_t covx_stride;
    int plane_stride, nlandmarks;
    const float *obs_zx, *obs_zy;
    float meas_var;
    const int32_t* live_in;
    int32_t* live_out;
    int32_t* cnt;          // [3]
    int phase;
    const uint32_t* cstamp;
    uint32_t stamp_now;
    int32_t* h_live;       // 8-byte word {cnt[phase], epoch} in mapped host memory
    int32_t* h_mark;       // ... and, written behind a system-scope fence, {mark, epoch}
    uint32_t epoch;
    uint32_t mark;         // the host's running count of classes appended to the list so far (sharded sessions: rows received)
    // survivor rows: the PRIOR rows of every class that is updated are first copied here (same strides; nullptr: not wanted)
    float* save_cov = nullptr;
    float* save_covx = nullptr;
};
// rows [n][5][plane_stride_in] (row_stride_in floats apart) -> means [n][2][Lp], classes, class rows [..][3][Lp]: neighbouring
// particles whose three covariance planes are equal bit for bit share a class (classes are numbered 0, 1, .. in particle
// order; all particles alike -> one class).  scratch: split_scratch_words(n) int32 words.  live[k] = k, cnt[phase] = number
// of classes (cnt[other] = 0), every class stamped stamp_now; h_live = {classes, epoch}.  A new epoch: cs.live and cs.cnt are
// the first list and the first of the three counts.
size_t split_scratch_words(int n);
// covx (written by a second launch, so that it may lie where the rows came from): the determinant terms of every class.
hipError_t launch_split_from_rows(hipStream_t stream, const float* rows, int64_t row_stride_in, int plane_stride_in, int nlandmarks,
                                  int n, float* mean, const ClassStore& cs, float meas_var, int32_t* h_live, uint32_t epoch, void* scratch);
// out row k = [means of particle idx[k] (or k) | the covariance planes of its class], nlandmarks columns of each plane
hipError_t launch_rows_from_split(hipStream_t stream, const float* mean, const ClassStore& cs, const int32_t* idx, int count,
                                  float* rows, int64_t row_stride, int plane_stride, int nlandmarks);
// Sharded sessions on the split layout.  A migrating particle travels as the same record whatever the layouts of the two ranks
// (pose, then five planes of nlandmarks values): launch_migrate_pack(.., split_cov, split_cls) reads it from the means and the
// class's covariance row, and this launch puts record p of `in` into staging row n + p of the means, with a class of its own —
// freelist[first + p], covariance planes and determinant terms filled in, appended to the list of classes in use (live[*cnt ..)).
// Class numbers for the arrivals come from a free list on the device: the classes no current particle belongs to, i.e. whose
// stamp is older than `min_live` — the stamp of the last update whose particles are the current ones.  At most n classes are in
// use and there are n + staging rows of them, so a list made anew holds at least as many numbers as a rank has staging rows,
// whatever else it holds: the HOST hands them out (entries [first, first + total) of the list go to this launch) and asks for
// a new list (launch_class_free_list, in front of the unpack) when the guaranteed part of the old one is used up.
//   fs: two int32 words on the device, zero before the first launch and zero again behind every launch.
hipError_t launch_class_free_list(hipStream_t stream, const uint32_t* cstamp, int nclasses, uint32_t min_live, int32_t* freelist,
                                  int32_t* fs);
// the arrivals' classes are stamped cs.stamp_now (= min_live: in use until the next update has said which of them have offspring)
hipError_t launch_migrate_unpack_split(hipStream_t stream, const float* in, int total, int n, float* pose, int64_t pose_ld, float* mean,
                                       const ClassStore& cs, int nlandmarks, float meas_var, const int32_t* freelist, int first);
// a frame without a landmark update: means and classes follow their particles (out[i] = in[anc[i]])
hipError_t launch_split_gather(hipStream_t stream, const float* mean_in, float* mean_out, const int32_t* cls_in, int32_t* cls_out,
                               int Lp, const int32_t* anc, int n, uint32_t* cstamp, uint32_t stamp_now);
// the classes alone follow their particles (split pages: the means follow through the page tables)
hipError_t launch_class_gather(hipStream_t stream, const int32_t* cls_in, int32_t* cls_out, const int32_t* anc, int n, uint32_t* cstamp,
                               uint32_t stamp_now);
// every particle: all landmarks "not seen yet", one class (a new epoch, as launch_split_from_rows)
hipError_t launch_split_reset(hipStream_t stream, float* mean, const ClassStore& cs, int n, int32_t* h_live, uint32_t epoch);

// ---- weights_kernels.hip (row A11; no reference counterpart): the weights of a frame
// carry / prev_resampled (optional): see logweight_kernel — the weights a frame without resample left behind
// cov (optional): the same launch carries the covariance classes' update of cov_bound classes in workgroups of its own — cov_update_body.h;
// cov->nlandmarks == 0: a frame without observations — only the list is brought up to date (classes whose last particle went
// with the frame's gather leave it: a sharded session may hand their numbers out again, and a number must not be listed twice)
hipError_t launch_logweight(hipStream_t stream, const float* score, const float* loglik, float gain, int n,
                            float* logw, float* block_max_scratch, float* d_max, const float* carry = nullptr,
                            const int32_t* prev_resampled = nullptr, const CovArgs* cov = nullptr, int cov_bound = 0);
int logweight_scratch_elems(int n);
int logweight_scratch_floats();   // size of block_max_scratch: block maxima + two words, zero-initialised once
hipError_t launch_quantise_weights(hipStream_t stream, const float* logw, const float* d_max, int n, uint64_t* wq,
                                   uint64_t* d_sum);

// ---- scan_kernels.hip (row A12): the integer CDF — staged over quantised weights, or quantise + tile scan in one pass
hipError_t launch_prefix_sum(hipStream_t stream, const uint64_t* in, int n, uint64_t* out, uint64_t* block_scratch);
int prefix_sum_scratch_elems(int n);
int scan_tile_count(int n);   // 2048-element tiles of the fused quantise + scan
// fused frame-loop form (the offsets then come straight from the tile-local scan: launch_offspring_from_scan).  The scan state is
// cdf_local[n] followed by tile_total[ntiles] | tile_s16[ntiles] | tile_q16[ntiles] (the last two only with a gate:
// carry != nullptr).  With a gate d_sum receives three values (total, S, Q) and d_shard_totals holds such triples.
// cov (optional; ungated, block maxima): the launch carries the covariance classes' update as launch_logweight does — for a
// frame whose front launch made the weights itself (launch_frame_front's FrontWeights), which has no weights' launch.
hipError_t launch_quantise_scan(hipStream_t stream, const float* logw, const float* d_max, const float* block_max,
                                int nblock_max, int n, uint64_t* cdf_local, uint64_t* tile_total, uint64_t* d_sum,
                                float* carry = nullptr, uint64_t* tile_s16 = nullptr, uint64_t* tile_q16 = nullptr,
                                unsigned int* ticket = nullptr, const CovArgs* cov = nullptr, int cov_bound = 0);

// ---- resample_kernels.hip (row A12): the ESS gate, the comb's offspring offsets, the ancestors on one GPU
// Where a resample stage reports roughly how many distinct ancestors it left: counter = one 8-byte-aligned pair of words
// (device, zeroed once, left zeroed), h_out = {count, n} in mapped host memory.
struct HeadsOut {
    unsigned int* counter = nullptr;
    int32_t* h_out = nullptr;
};
// The resample gate (ESS-gated resampling; oracle: orc_ess_resample).  frac_q16 = threshold * 65536, 0 = no gate
// (resample every frame).  Where the verdict goes: a device flag and, optionally, mapped host memory
// {int32 resampled, uint32 sequence number}.
// The gate's small device buffer, int32 words: [0] "the last resample stage did resample" (the flag logweight_kernel reads),
// [1] pad, [2] the ticket of quantise_scan_kernel's shard sums, [3] pad, [4..9] its three 64-bit accumulators (8-byte aligned)
enum { kGateFlagWord = 0, kGateTicketWord = 2, kGateBufWords = 16 };
struct GateOut {
    int32_t* d_flag = nullptr;
    int32_t* h_flag = nullptr;
    uint32_t seq = 0;
};
hipError_t launch_offspring_from_scan(hipStream_t stream, const uint64_t* cdf_local, const uint64_t* tile_total, int n,
                                      const uint64_t* d_base, const uint64_t* d_total, const uint64_t* d_shard_totals,
                                      int rank, int world, uint64_t seed, uint32_t frame, int64_t n_total,
                                      int32_t* first, uint32_t frac_q16 = 0, const GateOut& gate = GateOut());
hipError_t launch_offspring_offsets(hipStream_t stream, const uint64_t* cdf, int n, const uint64_t* d_base,
                                    const uint64_t* d_total, uint64_t seed, uint32_t frame, int64_t n_total,
                                    int32_t* first);
hipError_t launch_ancestors(hipStream_t stream, const int32_t* first_all, int64_t n_total, int64_t slot0, int nslots,
                            int32_t* anc);
// single GPU: offspring offsets + ancestors in one launch (n up to 8M; beyond that use the two launches above): every particle
// fills the run of slots it owns, [first[i], first[i + 1]) (offspring_fill_kernel)
bool ancestors_from_scan_fits(int n);
// survivors (optional): mark[i] = stamp for every particle i that is some slot's ancestor — the particles the resample kept
struct SurvivorOut {
    uint32_t* mark = nullptr;   // [n]
    uint32_t stamp = 0;
};
hipError_t launch_ancestors_from_scan(hipStream_t stream, const uint64_t* cdf_local, const uint64_t* tile_total, int n,
                                      uint64_t seed, uint32_t frame, int32_t* anc, uint32_t frac_q16 = 0,
                                      const GateOut& gate = GateOut(), const HeadsOut& heads = HeadsOut(),
                                      const SurvivorOut& survivors = SurvivorOut());

// ---- estimate_kernels.hip: what is read out of a population — the heaviest particle, the sums for the mean, the gathers
// index and value of the largest of v[0..n): lowest index on ties, NaN never wins, index 0 with nothing but -inf and NaN
hipError_t launch_argmax(hipStream_t stream, const float* v, int n, int32_t* idx_out, float* val_out);
// heaviest particle {logw, global id (int bits), x, y, theta} -> out5 (device) and optionally mapped host memory + seq
hipError_t launch_best_particle(hipStream_t stream, const float* v, int n, const float* px, const float* py,
                                const float* pth, int64_t first_id, float* out5, float* h_out5, uint32_t* h_seq,
                                uint32_t seq);
// exact fixed-point sums of the population {x, y: 2^-32; sin, cos of (theta - ref): 2^-30} -> out[4] (device), optionally
// mapped host memory + seq; acc[9] / ticket: zero-initialised device scratch the kernel leaves zeroed.
// carry != nullptr (a frame the resample gate kept): the weighted sums, out[9] = each of the four as two limbs
// (w16 * (V >> 21), w16 * (V & 0x1fffff)) and sum w16, with w16 = quantise(det_exp(carry[i])) >> 16
constexpr int kPoseSumsPlain = 4, kPoseSumsWeighted = 9;
hipError_t launch_pose_sums(hipStream_t stream, const float* x, const float* y, const float* th, const int32_t* idx,
                            int n, float ref_th, unsigned long long* acc, unsigned int* ticket, long long* out,
                            long long* h_out, uint32_t* h_seq, uint32_t seq, const float* carry = nullptr);
// exact second moments about `mean` (what the sums above gave): with DX = trunc((x - mean[0]) * 2^20), DY likewise and
// SS = trunc(sin_det(theta - mean[2]) * 2^20), the six sums of w * A * B for (A, B) = (DX,DX) (DX,DY) (DY,DY) (DX,SS) (DY,SS)
// (SS,SS), each as three limbs of the product P = A * B — out[3k] = sum w (P & 0x1fffff), out[3k + 1] = sum w ((P >> 21) & 0x1fffff),
// out[3k + 2] = sum w (P >> 42) — then out[kPoseMomentsD] = sum w and out[kPoseMomentsFlag] = how many particles lie outside the
// domain |x - mean[0]|, |y - mean[1]| < 2048 m (they count as zeros: the caller refuses the result).  w = 1, or with carry the w16 of
// launch_pose_sums.  acc[kPoseMoments] / ticket: zero-initialised device scratch the kernel leaves zeroed.
constexpr int kPoseMoments = 20, kPoseMomentsD = 18, kPoseMomentsFlag = 19;
hipError_t launch_pose_moments(hipStream_t stream, const float* x, const float* y, const float* th, const int32_t* idx,
                               int n, const float mean[3], unsigned long long* acc, unsigned int* ticket, long long* out,
                               long long* h_out, uint32_t* h_seq, uint32_t seq, const float* carry = nullptr);
// ---- modes_kernels.hip: the modes of a pose population (slam_pf_modes; specification: tests/_modes_spec.py).
// A cell is a key (ix, iy, b); the table is open addressing in device memory, one 64-byte line per cell, zero = empty.  Three
// launches: accumulate (the population once), score (one thread per occupied cell), select (one workgroup: the centres, their
// member sums, the hand-over, and the table cleared again for the next call).
struct ModesCell {
    unsigned long long key;      // 0: empty; else 1 + ((ix + 2^20) << 27 | (iy + 2^20) << 6 | b): ordered as (ix, iy, b) is
    unsigned long long sum[5];   // W, sum w FX, sum w FY, sum w S, sum w C (two's complement)
    unsigned long long score;    // sum of W over the neighbourhood (the score launch)
    unsigned long long pad;
};
constexpr int kModesSlots = 1 << 18;      // of the table; a power of two
constexpr int kModesMaxCells = 65536;     // distinct cells a call accepts
constexpr int kModesMaxBlocks = 512;      // of the accumulate launch: kModesMaxCells + 1 + its threads stay below kModesSlots (see there)
constexpr int kModesMax = 8;              // modes a call returns at most
// what the select launch hands over, 8-byte words: {particles outside the domain, cells inserted, Wtotal, n_modes}, then per mode
// {key, member cells, Wm, A_x, A_y, sum w S, sum w C}
constexpr int kModesHead = 4, kModesPer = 7, kModesWords = kModesHead + kModesMax * kModesPer;
struct ModesArgs {
    const float *x, *y, *th;     // [n] each
    const int32_t* idx;          // the pending gather (optional)
    const float* carry;          // the source of the 16-bit weights, one per SLOT (optional: w = 1)
    int n;
    float ref_theta, inv_cell;
    int hbins, max_modes;
    ModesCell* table;            // [kModesSlots], all zero between calls
    uint32_t* list;              // [kModesSlots] the slots in use, in the order they were claimed
    unsigned long long* ctrl;    // [3] {cells inserted (its low word), particles outside the domain, Wtotal}, zero between calls
    long long* out;              // [kModesWords] device memory
    long long* h_out;            // the same to mapped host memory behind *h_seq = seq (optional)
    uint32_t* h_seq;
    uint32_t seq;
};
hipError_t launch_modes(hipStream_t stream, const ModesArgs& a, int cus);
hipError_t launch_gather_f32(hipStream_t stream, const float* src, const int32_t* idx, int n, float* dst);
hipError_t launch_gather_map(hipStream_t stream, const float* in, float* out, int64_t in_row_stride,
                             int64_t out_row_stride, int in_plane_stride, int out_plane_stride, int nlandmarks,
                             const int32_t* idx, int n);

// ---- shard_kernels.hip: the resample of a sharded (multi-GPU) session — per-peer slot runs, offsets in the packed exchange buffers
enum { kMaxRanks = 16 };
struct MigratePlan {
    int64_t lo[kMaxRanks];       // pack: prefix count at the first particle sent to peer q (send_base); unpack: unused
    int32_t off[kMaxRanks + 1];  // running particle offset of peer q's run in the buffer (off[world] = total)
    int32_t world;
};
int shard_scan_words(int n);   // int32 words of scratch the two launchers below share
// host_plan / host_flag / seq (optional): also deliver the plan to mapped pinned host memory and release `seq`
hipError_t launch_ancestors_sharded(hipStream_t stream, const int32_t* first_all, int64_t n_total, int n, int rank,
                                    int world, int32_t* scratch, int32_t* plan, int32_t* src, int32_t* pose_idx,
                                    int32_t* host_plan, uint32_t* host_flag, uint32_t seq, int recv_cap,
                                    int32_t* host_heads = nullptr);
hipError_t launch_migrate_pack(hipStream_t stream, const int32_t* scratch, int n, const MigratePlan& plan,
                               const float* pose, int64_t pose_ld, const float* map, int64_t row_stride,
                               int plane_stride, int nlandmarks, float* out,
                               const int32_t* pt = nullptr, int nb = 0,
                               const float* split_cov = nullptr, const int32_t* split_cls = nullptr,
                               const PageGeom& geom = PageGeom());   // pt AND split_cls: split pages (means behind pt in pages of geom)
hipError_t launch_migrate_unpack(hipStream_t stream, const float* in, const MigratePlan& plan, int n, float* pose,
                                 int64_t pose_ld, float* map, int64_t row_stride, int plane_stride, int nlandmarks);

// ---- mapper_kernels.hip (reference: main.c:71-198, 271-354, 941-953)
hipError_t launch_clean_scan(hipStream_t s, const float* range, const float* cos_tab, const float* sin_tab, int nbeams,
                             float range_min, float usable, float* bx, float* by, int32_t* nscan);
hipError_t launch_transform(hipStream_t s, const float* bx, const float* by, const int32_t* nscan, float px, float py,
                            float ct, float st, float* tx, float* ty);
hipError_t launch_crop(hipStream_t s, const float* tx, const float* ty, const int32_t* nscan, float border,
                       const float* mx, const float* my, const int32_t* msize, int local_cap, float* lx, float* ly,
                       int32_t* lsize);
hipError_t launch_rasterise(hipStream_t s, const float* lx, const float* ly, const int32_t* lsize, float pixel, int ld,
                            int32_t* grid, slam_grid_meta* meta);
hipError_t launch_map_append(hipStream_t s, const float* hits, int nhits, const float* tx, const float* ty, float* mx,
                             float* my, int32_t* msize, int map_cap, float threshold);

}  // namespace slam
