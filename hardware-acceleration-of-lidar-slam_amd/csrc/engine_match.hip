// engine_match.hip — the matcher's side of the C ABI: the distance transform, the grid slots and the scan, the scorers of
// poses against a grid, and FastMatch in both forms (one call; the reference's chained pair as one round trip).

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "engine_internal.h"

using namespace slam;

namespace {

bool slot_ok(int slot) { return slot >= 0 && slot < SLAM_MAX_GRID_SLOTS; }

bool meta_ok(const slam_grid_meta* m)
{
    return m && m->rows >= 0 && m->cols >= 0 && m->ld >= m->cols && m->pixel > 0.0f &&
           (int64_t)m->rows * m->ld < (int64_t)0x7fffffff;
}

ScoreGrid score_grid(const GridSlot& g)
{
    ScoreGrid s;
    s.edt = g.d_edt;
    s.rows = g.meta.rows;
    s.cols = g.meta.cols;
    s.ld = g.meta.ld;
    s.ipix = 1 / g.meta.pixel;   // main.c:383 — one float division on the host
    s.min_x = g.meta.min_x;
    s.min_y = g.meta.min_y;
    return s;
}

// main.c:386-387, :424-426 — the lattice is laid out once around the input pose: X | Y | CT | ST of the 27 candidates into h_in,
// the three headings into th.  t steps x AND y, r steps theta.  Heading trig with the host libm, as the reference does
// (main.c:433-435).
void fill_lattice(const float pose[3], float t, float r, float* h_in, float th[3])
{
    th[0] = pose[2] - r;
    th[1] = pose[2];
    th[2] = pose[2] + r;
    const float xs[3] = { pose[0] - t, pose[0], pose[0] + t };
    const float ys[3] = { pose[1] - t, pose[1], pose[1] + t };
    for (int a = 0; a < 3; ++a) {
        const float c = cosf(th[a]), s = sinf(th[a]);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const int k = (a * 3 + i) * 3 + j;   // evaluation order theta, x, y (main.c:443-487)
                h_in[k] = xs[i];
                h_in[kLattice + k] = ys[j];
                h_in[2 * kLattice + k] = c;
                h_in[3 * kLattice + k] = s;
            }
    }
}

// main.c:549-563 — the first of the 27 scores below +inf that no other undercuts (strict '<' keeps the first of equals);
// -1: nothing beat +inf (NaN scores)
int first_min(const float* score)
{
    float best = INFINITY;
    int best_k = -1;
    for (int k = 0; k < kLattice; ++k)
        if (score[k] < best) {
            best = score[k];
            best_k = k;
        }
    return best_k;
}

}  // namespace

namespace slam_detail {

int check_score_inputs(slam_engine* e, int slot)
{
    if (!slot_ok(slot)) return SLAM_ERR_INVALID_ARG;
    if (!e->grid[slot].ready || e->nbeams < 0) return SLAM_ERR_NOT_READY;
    return SLAM_OK;
}

// The grid as the scorers of MANY poses want it: with the byte-per-cell copy (kernels.h: ScoreGrid::packed) when the grid
// has one.  The copy is made on the first such call after the grid changed — two small launches and ONE wait for their verdict
// (does the 256-entry table give every cell back bit for bit?), then nothing until the grid changes again.  Few poses (the
// one-wavefront-per-pose kernel, the lattice) keep the float grid.
int many_pose_grid(slam_engine* e, int slot, int nposes, ScoreGrid* out)
{
    GridSlot& g = e->grid[slot];
    *out = score_grid(g);
    if (nposes < kWaveMaxPoses || g.meta.rows < 8 || g.meta.cols < 16) return SLAM_OK;
    const int strip_bytes = 16 * ((g.meta.rows + 7) / 8 * 8);
    if (strip_bytes >= (1 << 24)) return SLAM_OK;   // 24-bit multiply in the scorer's cell offset
    if (g.packed_state == 0) {
        const size_t bytes = edt_packed_bytes(g.meta.rows, g.meta.cols);
        if (g.packed_buf.cap < bytes || g.table_buf.cap < 1024 + 8) {
            SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));   // an earlier launch may still read the old copy
            SLAM_HIP_TRY(e, g.packed_buf.ensure(bytes));
            SLAM_HIP_TRY(e, g.table_buf.ensure(1024 + 8));
        }
        uint32_t* flag = reinterpret_cast<uint32_t*>(g.table_buf.as<float>() + 256);
        SLAM_HIP_TRY(e, launch_edt_pack(e->stream, g.d_edt, g.meta.ld, g.meta.rows, g.meta.cols, g.packed_buf.as<uint8_t>(),
                                        g.table_buf.as<float>(), flag));
        uint32_t verdict[2] = { 0, 1 };
        SLAM_HIP_TRY(e, hipMemcpyAsync(verdict, flag, sizeof verdict, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
        g.packed_state = verdict[1] == 0 ? 1 : 2;
    }
    if (g.packed_state == 1) {
        out->packed = g.packed_buf.as<uint8_t>();
        out->table = g.table_buf.as<float>();
        out->strip_bytes = strip_bytes;
    }
    return SLAM_OK;
}

}  // namespace slam_detail

extern "C" {

/* ------------------------------------------------------------------ EDT */

int slam_edt_dev(slam_engine* e, const int32_t* d_occ, int ld, int rows, int cols, float cap, float* d_out)
{
    SLAM_ENTER(e);
    if (!d_occ || !d_out || rows < 0 || cols < 0 || ld < cols || !(cap >= 0.0f)) return SLAM_ERR_INVALID_ARG;
    if (ceilf(cap) > (float)EDT_MAX_RADIUS) return SLAM_ERR_CAPACITY;
    SLAM_HIP_TRY(e, launch_edt(e->stream, d_occ, ld, rows, cols, cap, d_out, e->prof_next(SLAM_PROF_EDT)));
    for (GridSlot& g : e->grid)   // an adopted grid rebuilt in place: its packed copy is stale
        if (g.ready && g.d_edt == d_out) g.packed_state = 0;
    return SLAM_OK;
}

int slam_edt_host(slam_engine* e, const int32_t* occ, int ld, int rows, int cols, float cap, float* out)
{
    SLAM_ENTER(e);
    if (!occ || !out || rows < 0 || cols < 0 || ld < cols || !(cap >= 0.0f)) return SLAM_ERR_INVALID_ARG;
    if (ceilf(cap) > (float)EDT_MAX_RADIUS) return SLAM_ERR_CAPACITY;
    if (rows == 0 || cols == 0) return SLAM_OK;
    const size_t cells = (size_t)rows * ld;
    SLAM_HIP_TRY(e, e->host_io[0].ensure(cells * sizeof(int32_t)));
    SLAM_HIP_TRY(e, e->host_io[1].ensure(cells * sizeof(float)));
    SLAM_HIP_TRY(e, hipMemcpyAsync(e->host_io[0].p, occ, cells * sizeof(int32_t), hipMemcpyHostToDevice, e->stream));
    SLAM_HIP_TRY(e, launch_edt(e->stream, e->host_io[0].as<int32_t>(), ld, rows, cols, cap, e->host_io[1].as<float>()));
    // only the rows x cols rectangle belongs to the caller's output (cells outside keep their content, Q7)
    SLAM_HIP_TRY(e, hipMemcpy2DAsync(out, (size_t)ld * sizeof(float), e->host_io[1].p, (size_t)ld * sizeof(float),
                                     (size_t)cols * sizeof(float), (size_t)rows, hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return SLAM_OK;
}

/* ------------------------------------------------------------------ grids + scan */

int slam_grid_upload_host(slam_engine* e, int slot, const int32_t* occ, const slam_grid_meta* meta, float cap,
                          float* edt_out)
{
    SLAM_ENTER(e);
    if (!slot_ok(slot) || !occ || !meta_ok(meta) || !(cap >= 0.0f)) return SLAM_ERR_INVALID_ARG;
    if (ceilf(cap) > (float)EDT_MAX_RADIUS) return SLAM_ERR_CAPACITY;
    GridSlot& g = e->grid[slot];
    const size_t cells = (size_t)(meta->rows > 0 ? meta->rows : 1) * meta->ld;
    SLAM_HIP_TRY(e, g.occ_buf.ensure(cells * sizeof(int32_t)));
    SLAM_HIP_TRY(e, g.edt_buf.ensure(cells * sizeof(float)));
    if (meta->rows > 0) {
        SLAM_HIP_TRY(e, hipMemcpyAsync(g.occ_buf.p, occ, (size_t)meta->rows * meta->ld * sizeof(int32_t), hipMemcpyHostToDevice,
                                       e->stream));
        SLAM_HIP_TRY(e, launch_edt(e->stream, g.occ_buf.as<int32_t>(), meta->ld, meta->rows, meta->cols, cap,
                                   g.edt_buf.as<float>()));
    }
    g.meta = *meta;
    g.d_edt = g.edt_buf.as<float>();
    g.ready = true;
    g.packed_state = 0;
    if (edt_out && meta->rows > 0 && meta->cols > 0) {
        SLAM_HIP_TRY(e, hipMemcpy2DAsync(edt_out, (size_t)meta->ld * sizeof(float), g.edt_buf.p,
                                         (size_t)meta->ld * sizeof(float), (size_t)meta->cols * sizeof(float),
                                         (size_t)meta->rows, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
    return SLAM_OK;
}

int slam_grid_set_dev(slam_engine* e, int slot, const float* d_edt, const slam_grid_meta* meta)
{
    SLAM_ENTER(e);
    if (!slot_ok(slot) || !d_edt || !meta_ok(meta)) return SLAM_ERR_INVALID_ARG;
    GridSlot& g = e->grid[slot];
    g.meta = *meta;
    g.d_edt = d_edt;
    g.ready = true;
    g.packed_state = 0;   // the scorers' packed copy is made from the new contents on their next call
    return SLAM_OK;
}

int slam_grid_set_meta(slam_engine* e, int slot, const slam_grid_meta* meta)
{
    SLAM_ENTER(e);
    if (!slot_ok(slot) || !meta_ok(meta)) return SLAM_ERR_INVALID_ARG;
    GridSlot& g = e->grid[slot];
    if (!g.ready) return SLAM_ERR_NOT_READY;
    if (meta->rows != g.meta.rows || meta->cols != g.meta.cols || meta->ld != g.meta.ld) return SLAM_ERR_INVALID_ARG;
    g.meta = *meta;
    return SLAM_OK;
}

int slam_grid_packed_state(slam_engine* e, int slot, int* state)
{
    SLAM_ENTER(e);
    if (!slot_ok(slot) || !state) return SLAM_ERR_INVALID_ARG;
    if (!e->grid[slot].ready) return SLAM_ERR_NOT_READY;
    *state = e->grid[slot].packed_state;
    return SLAM_OK;
}

int slam_scan_upload_host(slam_engine* e, const float* bx, const float* by, int nbeams)
{
    SLAM_ENTER(e);
    if (nbeams < 0 || (nbeams > 0 && (!bx || !by))) return SLAM_ERR_INVALID_ARG;
    if (nbeams > SLAM_MAX_BEAMS) return SLAM_ERR_CAPACITY;
    float* d = e->scan_buf.as<float>();
    if (nbeams > 0) {
        // pinned staging -> ONE host-to-device copy per frame (bx | by back to back)
        float* h = e->stage_acquire();
        memcpy(h, bx, sizeof(float) * nbeams);
        memcpy(h + nbeams, by, sizeof(float) * nbeams);
        SLAM_HIP_TRY(e, hipMemcpyAsync(d, h, sizeof(float) * 2 * nbeams, hipMemcpyHostToDevice, e->stream));
        SLAM_HIP_TRY(e, e->stage_release(h));
    }
    e->d_bx = d;
    e->d_by = d + nbeams;
    e->nbeams = nbeams;
    e->sight_bins = 0;   // (the sight table belonged to the scan before)
    return SLAM_OK;
}

int slam_scan_set_dev(slam_engine* e, const float* d_bx, const float* d_by, int nbeams)
{
    SLAM_ENTER(e);
    if (nbeams < 0 || (nbeams > 0 && (!d_bx || !d_by))) return SLAM_ERR_INVALID_ARG;
    if (nbeams > SLAM_MAX_BEAMS) return SLAM_ERR_CAPACITY;
    e->d_bx = d_bx;
    e->d_by = d_by;
    e->nbeams = nbeams;
    e->sight_bins = 0;
    return SLAM_OK;
}

/* ------------------------------------------------------------------ score */

int slam_score_poses_cs_dev(slam_engine* e, int slot, const float* d_x, const float* d_y, const float* d_ct,
                            const float* d_st, int nposes, float* d_score, int32_t* d_count)
{
    SLAM_ENTER(e);
    if (nposes < 0 || (nposes > 0 && (!d_x || !d_y || !d_ct || !d_st || !d_score || !d_count)))
        return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, nposes, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_score_poses(e->stream, sg, e->d_bx, e->d_by, e->nbeams, d_x, d_y, d_ct, d_st,
                                       nposes, d_score, d_count, e->prof_next(SLAM_PROF_SCORE)));
    return SLAM_OK;
}

int slam_score_poses_dev(slam_engine* e, int slot, const float* d_x, const float* d_y, const float* d_theta,
                         int nposes, float* d_score, int32_t* d_count)
{
    SLAM_ENTER(e);
    if (nposes < 0 || (nposes > 0 && (!d_x || !d_y || !d_theta || !d_score || !d_count))) return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, nposes, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_score_poses(e->stream, sg, e->d_bx, e->d_by, e->nbeams, d_x, d_y, d_theta,
                                       nullptr, nposes, d_score, d_count, e->prof_next(SLAM_PROF_SCORE)));
    return SLAM_OK;
}

static int score_host_common(slam_engine* e, int slot, const float* x, const float* y, const float* a,
                             const float* b, int nposes, float* score, int32_t* count)
{
    if (nposes < 0 || (nposes > 0 && (!x || !y || !a || !score || !count))) return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    if (nposes == 0) return SLAM_OK;
    const size_t bytes = sizeof(float) * (size_t)nposes;
    const float* src[4] = { x, y, a, b };
    for (int k = 0; k < 6; ++k) SLAM_HIP_TRY(e, e->host_io[k].ensure(bytes));
    for (int k = 0; k < 4; ++k)
        if (src[k]) SLAM_HIP_TRY(e, hipMemcpyAsync(e->host_io[k].p, src[k], bytes, hipMemcpyHostToDevice, e->stream));
    ScoreGrid sg;
    if (int rc = many_pose_grid(e, slot, nposes, &sg)) return rc;
    SLAM_HIP_TRY(e, launch_score_poses(e->stream, sg, e->d_bx, e->d_by, e->nbeams,
                                       e->host_io[0].as<float>(), e->host_io[1].as<float>(), e->host_io[2].as<float>(),
                                       b ? e->host_io[3].as<float>() : nullptr, nposes, e->host_io[4].as<float>(),
                                       e->host_io[5].as<int32_t>()));
    SLAM_HIP_TRY(e, hipMemcpyAsync(score, e->host_io[4].p, bytes, hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipMemcpyAsync(count, e->host_io[5].p, bytes, hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return SLAM_OK;
}

int slam_score_poses_cs_host(slam_engine* e, int slot, const float* x, const float* y, const float* ct,
                             const float* st, int nposes, float* score, int32_t* count)
{
    SLAM_ENTER(e);
    if (nposes > 0 && !st) return SLAM_ERR_INVALID_ARG;
    return score_host_common(e, slot, x, y, ct, st, nposes, score, count);
}

int slam_score_poses_host(slam_engine* e, int slot, const float* x, const float* y, const float* theta, int nposes,
                          float* score, int32_t* count)
{
    SLAM_ENTER(e);
    return score_host_common(e, slot, x, y, theta, nullptr, nposes, score, count);
}

int slam_pose_hits_host(slam_engine* e, int slot, float x, float y, float ct, float st, float* hits, int32_t* count)
{
    SLAM_ENTER(e);
    if (!hits || !count) return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    float* d_in = e->fm_buf.as<float>();
    float* d_out = d_in + kFmIn;
    float* h_in = e->h_fm;
    float* h_out = e->h_fm + kFmIn;
    h_in[4 * kLattice + 0] = x;
    h_in[4 * kLattice + 1] = y;
    h_in[4 * kLattice + 2] = ct;
    h_in[4 * kLattice + 3] = st;
    SLAM_HIP_TRY(e, hipMemcpyAsync(d_in + 4 * kLattice, h_in + 4 * kLattice, 4 * sizeof(float), hipMemcpyHostToDevice,
                                   e->stream));
    SLAM_HIP_TRY(e, launch_pose_hits(e->stream, score_grid(e->grid[slot]), e->d_bx, e->d_by, e->nbeams, d_in + 4 * kLattice,
                                     d_out + 2 * kLattice + 1, reinterpret_cast<int32_t*>(d_out + 2 * kLattice)));
    SLAM_HIP_TRY(e, hipMemcpyAsync(h_out + 2 * kLattice, d_out + 2 * kLattice, sizeof(float) * (1 + (size_t)e->nbeams),
                                   hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    memcpy(count, h_out + 2 * kLattice, sizeof(int32_t));
    if (*count > 0) memcpy(hits, h_out + 2 * kLattice + 1, sizeof(float) * (size_t)*count);
    return SLAM_OK;
}

}  // extern "C"

// ---- internal entry points shared with mapper.hip (C++ linkage, declared in engine_internal.h)
slam::ScoreGrid slam_engine_score_grid(const slam_engine* e, int slot) { return score_grid(e->grid[slot]); }

int slam_engine_fastmatch(slam_engine* e, int slot, const float* d_bx, const float* d_by, int nbeams_max,
                          const int32_t* d_nbeams, const float pose[3], const float res[3], float out_pose[3],
                          float* best_hits, int32_t* best_hits_size, float* best_score, float* d_hits_persist)
{
    float* h_in = e->h_fm;
    float* h_out = e->h_fm + kFmIn;
    float th[3];
    fill_lattice(pose, res[0], res[2], h_in, th);   // res[1] is never read
    float* d_out = e->fm_buf.as<float>() + kFmIn;
    const ScoreGrid g = score_grid(e->grid[slot]);
    // zero-copy I/O: the kernels read the 27 candidates from, and deliver their result to, pinned host memory
    // mapped into the device; the host waits for the arrival flag instead of a copy + stream synchronisation
    volatile uint32_t* h_flag = reinterpret_cast<volatile uint32_t*>(e->h_fm + kFmIn + kFmOut);
    const uint32_t seq = ++e->fm_seq;
    SLAM_HIP_TRY(e, launch_lattice(e->stream, g, d_bx, d_by, nbeams_max, d_nbeams, e->d_hfm, e->fm_work.as<float>(), d_out,
                                   d_hits_persist, e->d_hfm + kFmIn, reinterpret_cast<uint32_t*>(e->d_hfm + kFmIn + kFmOut), seq));
    if (int rc = slam_engine_wait_flag(e, nullptr, h_flag, seq, "lattice result flag")) return rc;

    const int best_k = first_min(h_out);
    if (best_k >= 0) {
        out_pose[0] = h_in[best_k];
        out_pose[1] = h_in[kLattice + best_k];
        out_pose[2] = th[best_k / 9];
        memcpy(best_hits_size, h_out + kLattice + best_k, sizeof(int32_t));
    } else {   // nothing beat +inf (NaN scores): the reference returns the input pose, size untouched
        out_pose[0] = pose[0];
        out_pose[1] = pose[1];
        out_pose[2] = pose[2];
    }
    // the caller's hit buffer ends up exactly as the reference's shared scratch does: the
    // prefix every candidate overwrote, last writer wins; entries beyond the longest candidate untouched
    int32_t maxc;
    memcpy(&maxc, h_out + 2 * kLattice, sizeof maxc);
    if (maxc > 0 && best_hits) memcpy(best_hits, h_out + 2 * kLattice + 1, sizeof(float) * (size_t)maxc);
    if (best_score) *best_score = best_k >= 0 ? h_out[best_k] : INFINITY;
    return SLAM_OK;
}

// main.c:901-924 as ONE round trip: FastMatch(pose, res1) on grid slot1, then FastMatch2(its result, res2) on grid slot2 — the
// second call's lattice is laid out on the device around the first call's best candidate, so the host waits once instead of
// twice (a call is bound by that wait: 30 us, of which the kernels are a third).  What the reference computes with libm
// stays on the host: the first call's best heading is one of three values, so the second call's three headings are among
// NINE known before the launch; the host sends the cosines and sines of all nine and the device picks its three.  The
// candidates' x and y are one float add / subtract each, the same on the device.  The host repeats both arg-min decisions
// on the scores it receives (strict '<', the first of equals; nothing below +inf: the input pose and the previous size) —
// the device's choice of the first call's winner is the same computation on the same floats.
int slam_engine_fastmatch_pair(slam_engine* e, int slot1, int slot2, const float* d_bx, const float* d_by, int nbeams_max,
                               const int32_t* d_nbeams, const float pose[3], const float res1[3], const float res2[3],
                               float out_pose[3], int32_t* best_hits_size, float* d_hits_persist)
{
    const float t1 = res1[0], r1 = res1[2], t2 = res2[0], r2 = res2[2];
    float* h_in = e->h_fm;
    float* h_out2 = e->h_fm + kFmIn;
    float* h_pair_in = e->h_fm + kFmIn + kFmOut + 4;
    float* h_out1 = h_pair_in + kFmPairIn;
    float th1[3], th2[3][3];
    fill_lattice(pose, t1, r1, h_in, th1);
    for (int a = 0; a < 3; ++a) {
        th2[a][0] = th1[a] - r2;
        th2[a][1] = th1[a];
        th2[a][2] = th1[a] + r2;
        for (int b = 0; b < 3; ++b) {
            h_pair_in[a * 3 + b] = cosf(th2[a][b]);
            h_pair_in[9 + a * 3 + b] = sinf(th2[a][b]);
        }
    }
    h_pair_in[18] = t2;
    float* d_out1 = e->fm_buf.as<float>();           // the first call's scores | counts | maxcount (kFmIn floats are room enough)
    float* d_out2 = e->fm_buf.as<float>() + kFmIn;   // the second call's
    float* work1 = e->fm_work.as<float>();
    float* work2 = work1 + (size_t)kLattice * SLAM_MAX_BEAMS;
    volatile uint32_t* h_flag = reinterpret_cast<volatile uint32_t*>(e->h_fm + kFmIn + kFmOut);
    const uint32_t seq = ++e->fm_seq;
    SLAM_HIP_TRY(e, launch_lattice_pair(e->stream, score_grid(e->grid[slot1]), score_grid(e->grid[slot2]), d_bx, d_by, nbeams_max, d_nbeams, e->d_hfm,
                                        e->d_hfm + kFmIn + kFmOut + 4, work1, work2, d_out1, d_out2, d_hits_persist,
                                        e->d_hfm + kFmIn + kFmOut + 4 + kFmPairIn, e->d_hfm + kFmIn,
                                        reinterpret_cast<uint32_t*>(e->d_hfm + kFmIn + kFmOut), seq));
    if (int rc = slam_engine_wait_flag(e, nullptr, h_flag, seq, "lattice result flag")) return rc;
    // the first call: nothing below +inf: the input pose, size untouched
    const int k1 = first_min(h_out1);
    float p1[3] = { pose[0], pose[1], pose[2] };
    int a1 = 1;
    if (k1 >= 0) {
        p1[0] = h_in[k1];
        p1[1] = h_in[kLattice + k1];
        a1 = k1 / 9;
        p1[2] = th1[a1];
        memcpy(best_hits_size, h_out1 + kLattice + k1, sizeof(int32_t));
    }
    // the second call, laid out around p1 (the device built the same table around the same candidate)
    const float xs2[3] = { p1[0] - t2, p1[0], p1[0] + t2 };
    const float ys2[3] = { p1[1] - t2, p1[1], p1[1] + t2 };
    const int k2 = first_min(h_out2);
    if (k2 >= 0) {
        out_pose[0] = xs2[(k2 / 3) % 3];
        out_pose[1] = ys2[k2 % 3];
        out_pose[2] = th2[a1][k2 / 9];
        memcpy(best_hits_size, h_out2 + kLattice + k2, sizeof(int32_t));
    } else {
        out_pose[0] = p1[0];
        out_pose[1] = p1[1];
        out_pose[2] = p1[2];
    }
    return SLAM_OK;
}

extern "C" {

int slam_fastmatch_host(slam_engine* e, int slot, const float pose[3], const float res[3], float out_pose[3],
                        float* best_hits, int32_t* best_hits_size, float* best_score)
{
    SLAM_ENTER(e);
    if (!pose || !res || !out_pose || !best_hits || !best_hits_size) return SLAM_ERR_INVALID_ARG;
    if (int rc = check_score_inputs(e, slot)) return rc;
    return slam_engine_fastmatch(e, slot, e->d_bx, e->d_by, e->nbeams, nullptr, pose, res, out_pose, best_hits,
                                 best_hits_size, best_score, nullptr);
}

}  // extern "C"
