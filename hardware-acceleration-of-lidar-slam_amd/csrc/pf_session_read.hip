// pf_session_read.hip — what a host reads back from a session: the heaviest particle, the posterior mean and the spread about it
// (slam_pf_best, slam_pf_mean, slam_pf_spread), poses, map rows and evidence copied out, the device views, the layout in force; the pending gather of the last
// resample is applied on the way.  On a sharded session the copying calls are collective (collective_result).

#include <math.h>
#include <string.h>

#include <vector>

#include "pf_session.h"

namespace slam::session {
namespace {

// Every slam_pf_* call on a sharded session is collective: a rank that fails one alone (an error of its own, not a verdict
// every rank reaches together) must not leave the others waiting inside it — it gives up for good (comm_abort), the peers get
// SLAM_ERR_COMM at once instead of after SLAM_COMM_TIMEOUT_S.
int collective_result(slam_pf* pf, int rc)
{
    // (argument checks come before anything collective and are the same on every rank of a sane host: no abort for those)
    if (rc != SLAM_OK && rc != SLAM_ERR_INVALID_ARG && rc != SLAM_ERR_NOT_READY && pf && pf->comm) (void)comm_abort(pf->comm);
    return rc;
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

// every rank's `bytes` of res_dev -> h_all[world][bytes] on the host (one GPU: its own): an all-gather, a copy and a wait
int shares_to_host(slam_pf* pf, size_t bytes, void* h_all)
{
    const void* src = pf->res_dev;
    if (pf->comm) {
        if (int rc = comm_all_gather(pf->comm, pf->res_dev, pf->res_all, bytes)) return rc;
        src = pf->res_all;
    }
    SLAM_HIP_TRY(pf->e, hipMemcpyAsync(h_all, src, bytes * (size_t)pf->world, hipMemcpyDeviceToHost, pf->e->stream));
    return wait_stream(pf);
}

// the K integer sums pose_sums_kernel or pose_moments_kernel left in res_dev, added over the ranks: in any order they give the single-GPU bits (every
// limb sum of the whole population fits 64 bits)
int summed_shares(slam_pf* pf, int K, long long* total)
{
    std::vector<long long> all((size_t)K * (size_t)pf->world);
    if (int rc = shares_to_host(pf, (size_t)K * sizeof(long long), all.data())) return rc;
    for (int q = 0; q < pf->world; ++q)
        for (int k = 0; k < K; ++k) total[k] += all[(size_t)K * (size_t)q + k];
    return SLAM_OK;
}

int pf_best(slam_pf* pf, float pose[3], float* logw, int32_t* index)
{
    if (!pf || !pose) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    if (pf->reseeded) {   // pose[cur] is the reseeded population: the last frame's log-weights belong to none of it
        snprintf(e->err, sizeof e->err, "the population was reseeded (slam_pf_known_map_reseed): the last frame's log-weights no longer "
                                        "belong to the poses; the heaviest particle is known again after the next slam_pf_step");
        return SLAM_ERR_NOT_READY;
    }
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
        std::vector<float> all(5 * (size_t)pf->world);
        if (int rc = shares_to_host(pf, 5 * sizeof(float), all.data())) return rc;
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

// What slam_pf_mean and slam_pf_spread share: the poses behind the pending gather, whether the mean is the weighted one, the mean
struct MeanOf {
    const float* x = nullptr;
    const int32_t* idx = nullptr;
    bool weighted = false;
    PoseMean m;
};

int mean_of(slam_pf* pf, float ref_theta, MeanOf* out)
{
    slam_engine* e = pf->e;
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    const size_t sn = (size_t)pf->n;
    const float* x = nullptr;
    const int32_t* idx = nullptr;
    if (int rc = ancestor_poses(pf, &x, &idx)) return rc;
    out->x = x;
    out->idx = idx;
    const float *y = x + sn, *th = x + 2 * sn;
    unsigned int* ticket = reinterpret_cast<unsigned int*>(pf->sums_acc + kPoseSumsWeighted);
    // A frame the resample gate kept (its verdict is on its way to mapped host memory: wait for it) left unequal weights:
    // the weighted mean of DESIGN.md section 7.  Nine sums, so they come back by a copy, not through the mapped payload.
    int resampled = 1;
    if (pf->gated && pf->has_anc)
        if (int rc = slam_resample_happened_host(e, &resampled)) return rc;
    if (!resampled) {
        SLAM_HIP_TRY(e, launch_pose_sums(e->stream, x, y, th, idx, pf->n, ref_theta, pf->sums_acc, ticket,
                                         reinterpret_cast<long long*>(pf->res_dev), nullptr, nullptr, 0, e->carry_buf.as<float>()));
        long long w[kPoseSumsWeighted] = { 0 };
        if (int rc = summed_shares(pf, kPoseSumsWeighted, w)) return rc;
        if (w[8] > 0) {   // (no weight at all: log-weights that are not numbers — the plain mean below)
            out->weighted = true;
            out->m = mean_from_weighted_sums(w, ref_theta);
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
        if (int rc = summed_shares(pf, 4, sums)) return rc;
    }
    out->weighted = false;
    out->m = mean_from_plain_sums(sums, pf->n_total, ref_theta);
    return SLAM_OK;
}

int pf_mean(slam_pf* pf, float ref_theta, float pose[3])
{
    if (!pf || !pose) return SLAM_ERR_INVALID_ARG;
    MeanOf mo;
    if (int rc = mean_of(pf, ref_theta, &mo)) return rc;
    memcpy(pose, mo.m.pose, sizeof mo.m.pose);
    return SLAM_OK;
}

// the mean (mean_of), then the second moments about it in a launch of their own: one GPU — the sums land in mapped host memory;
// sharded — the mean is the global one by now, and the moments' shares are added over the ranks like the mean's
int pf_spread(slam_pf* pf, float ref_theta, float pose[3], float cov[6], float* heading_r)
{
    if (!pf || !pose || !cov || !heading_r) return SLAM_ERR_INVALID_ARG;
    MeanOf mo;
    if (int rc = mean_of(pf, ref_theta, &mo)) return rc;
    slam_engine* e = pf->e;
    const size_t sn = (size_t)pf->n;
    const float* carry = mo.weighted ? e->carry_buf.as<float>() : nullptr;
    unsigned int* ticket = reinterpret_cast<unsigned int*>(pf->moments_acc + kPoseMoments);
    long long m[kPoseMoments] = { 0 };
    if (!pf->comm) {
        const uint32_t seq = ++pf->res_seq;
        SLAM_HIP_TRY(e, launch_pose_moments(e->stream, mo.x, mo.x + sn, mo.x + 2 * sn, mo.idx, pf->n, mo.m.pose, pf->moments_acc, ticket,
                                            reinterpret_cast<long long*>(pf->res_dev), reinterpret_cast<long long*>(dev_word(pf, RES_MOMENTS)),
                                            reinterpret_cast<uint32_t*>(dev_word(pf, RES_SEQ)), seq, carry));
        if (int rc = wait_result(pf, seq)) return rc;
        memcpy(m, host_word(pf, RES_MOMENTS), sizeof m);
    } else {
        SLAM_HIP_TRY(e, launch_pose_moments(e->stream, mo.x, mo.x + sn, mo.x + 2 * sn, mo.idx, pf->n, mo.m.pose, pf->moments_acc, ticket,
                                            reinterpret_cast<long long*>(pf->res_dev), nullptr, nullptr, 0, carry));
        if (int rc = summed_shares(pf, kPoseMoments, m)) return rc;
    }
    return slam_engine_spread_result(e, mo.m, m, pose, cov, heading_r);
}

// the modes of the population behind the pending gather: the weights by the rules of mean_of (the gate's on a frame it kept,
// else w = 1), three launches, the raw words through mapped host memory.  One GPU only.
int pf_modes(slam_pf* pf, float ref_theta, float cell, int hbins, int max_modes, slam_pf_mode* modes, int* n_modes, int* cells)
{
    if (!pf || !modes || !n_modes || !cells) return SLAM_ERR_INVALID_ARG;
    slam_engine* e = pf->e;
    if (pf->comm) {
        snprintf(e->err, sizeof e->err, "the modes of a sharded population are not built (cells would have to be added over the ranks): "
                                        "one GPU only");
        return SLAM_ERR_INVALID_ARG;
    }
    SLAM_HIP_TRY(e, hipSetDevice(e->device));
    const size_t sn = (size_t)pf->n;
    const float* x = nullptr;
    const int32_t* idx = nullptr;
    if (int rc = ancestor_poses(pf, &x, &idx)) return rc;
    int resampled = 1;
    if (pf->gated && pf->has_anc)
        if (int rc = slam_resample_happened_host(e, &resampled)) return rc;
    long long raw[kModesWords];
    for (int pass = resampled ? 1 : 0; pass < 2; ++pass) {   // pass 0: weighted; pass 1: plain (also where no particle has any weight)
        const uint32_t seq = ++pf->res_seq;
        const long long* d_raw = nullptr;
        if (int rc = slam_engine_modes_launch(e, x, x + sn, x + 2 * sn, idx, pass == 0 ? e->carry_buf.as<float>() : nullptr, pf->n, ref_theta,
                                              cell, hbins, max_modes, reinterpret_cast<long long*>(dev_word(pf, RES_MODES)),
                                              reinterpret_cast<uint32_t*>(dev_word(pf, RES_SEQ)), seq, &d_raw)) {
            --pf->res_seq;   // (nothing was launched that would write it)
            return rc;
        }
        if (int rc = wait_result(pf, seq)) return rc;
        memcpy(raw, host_word(pf, RES_MODES), sizeof raw);
        if (!(pass == 0 && raw[0] == 0 && raw[2] == 0)) break;
    }
    return slam_engine_modes_result(e, raw, ref_theta, cell, modes, n_modes, cells, nullptr);
}

int pf_get_poses_host(slam_pf* pf, float* x, float* y, float* theta)
{
    if (!pf || !x || !y || !theta) return SLAM_ERR_INVALID_ARG;
    const size_t n = (size_t)pf->n;
    float* tmp = pf->pose[1 - pf->cur];   // the other buffer is free between frames
    float* out[3] = { x, y, theta };
    const float* p = nullptr;
    const int32_t* idx = nullptr;
    if (int rc = ancestor_poses(pf, &p, &idx)) return rc;
    for (int k = 0; k < 3; ++k)
        if (int rc = gathered_copy_out(pf, p + k * n, idx, out[k], tmp)) return rc;
    return SLAM_OK;
}

// dense rows [count][5][Lp] of the particles idx[0 .. count) (nullptr: 0 .. count - 1) of a session on pages, split or split pages
hipError_t rows_of(const slam_pf* pf, const int32_t* idx, int count, float* dense)
{
    hipStream_t s = pf->e->stream;
    const int64_t stride = pf->row_stride();
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
        if (hipMalloc((void**)&dense, (size_t)pf->row_stride() * n * 4) != hipSuccess) return SLAM_ERR_HIP;
        if (rows_of(pf, idx, pf->n, dense) != hipSuccess) rc = SLAM_ERR_HIP;
        src = dense;
    } else if (idx) {               // -> the spare row buffer
        rc = slam_gather_map_dev(pf->e, src, pf->map[1 - pf->map_cur], pf->row_stride(), pf->row_stride(), pf->Lp, pf->Lp, pf->L, idx, pf->n);
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
    SLAM_HIP_TRY(e, hipMalloc((void**)&dense, (size_t)pf->row_stride() * (size_t)count * 4));
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
            ok(launch_gather_map(e->stream, pf->map[pf->map_cur], dense, pf->row_stride(), pf->row_stride(), pf->Lp, pf->Lp, pf->L, src,
                                 count), "gather_map");
    }
    if (rc == SLAM_OK) ok(hipStreamSynchronize(e->stream), "hipStreamSynchronize");
    if (rc == SLAM_OK) ok(hipMemcpy2D(rows, L * 4, dense, Lp * 4, L * 4, 5 * (size_t)count, hipMemcpyDeviceToHost), "hipMemcpy2D");
    (void)hipFree(dense);
    return rc;
}

}  // namespace
}  // namespace slam::session

using namespace slam;
using namespace slam::session;

extern "C" {

int slam_pf_best(slam_pf* pf, float pose[3], float* logw, int32_t* index) { return collective_result(pf, pf_best(pf, pose, logw, index)); }
int slam_pf_mean(slam_pf* pf, float ref_theta, float pose[3]) { return collective_result(pf, pf_mean(pf, ref_theta, pose)); }
int slam_pf_spread(slam_pf* pf, float ref_theta, float pose[3], float cov[6], float* heading_r) { return collective_result(pf, pf_spread(pf, ref_theta, pose, cov, heading_r)); }
int slam_pf_modes(slam_pf* pf, float ref_theta, float cell, int hbins, int max_modes, slam_pf_mode* modes, int* n_modes, int* cells)
{
    return pf_modes(pf, ref_theta, cell, hbins, max_modes, modes, n_modes, cells);   // (never collective: sharded sessions are refused)
}
int slam_pf_get_poses_host(slam_pf* pf, float* x, float* y, float* theta) { return collective_result(pf, pf_get_poses_host(pf, x, y, theta)); }
int slam_pf_get_map_host(slam_pf* pf, float* rows) { return collective_result(pf, pf_get_map_host(pf, rows)); }
int slam_pf_get_map_rows_host(slam_pf* pf, const int32_t* particle, int count, float* rows) { return collective_result(pf, pf_get_map_rows_host(pf, particle, count, rows)); }

int slam_pf_is_paged(const slam_pf* pf) { return pf && pf->paged ? 1 : 0; }

int slam_pf_layout(const slam_pf* pf)
{
    if (!pf || !pf->L) return SLAM_MAP_ROWS;
    return pf->paged ? (pf->split ? SLAM_MAP_SPLIT_PAGES : SLAM_MAP_PAGES) : pf->split ? SLAM_MAP_SPLIT : SLAM_MAP_ROWS;
}

int slam_pf_device_view(slam_pf* pf, slam_pf_view* out)
{
    if (!pf || !out) return SLAM_ERR_INVALID_ARG;
    if (int rc = settle_means(pf)) return rc;
    out->pose = pf->pose[pf->cur];
    const bool rows = pf->L && !pf->paged && !pf->split;   // pages and split maps have no rows to look at: slam_pf_set_map_dev
    out->map = rows ? pf->map[pf->map_cur] : nullptr;
    out->map_spare = rows ? pf->map[1 - pf->map_cur] : nullptr;
    out->anc = pf->has_anc ? pf->anc[pf->cur] : nullptr;
    out->row_stride = pf->row_stride();
    out->plane_stride = pf->Lp;
    out->map_rows = pf->cap;
    out->score = pf->has_anc ? pf->score : nullptr;
    out->logw = pf->has_anc ? pf->logw : nullptr;
    out->loglik = pf->has_anc && pf->last_ekf && pf->e->ll_n == pf->n ? pf->e->ll_buf.as<float>() : nullptr;
    out->count = pf->has_anc ? pf->count : nullptr;
    return SLAM_OK;
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

int slam_pf_assoc_device_view(slam_pf* pf, const uint8_t** assoc, int32_t* assoc_stride, const int32_t** stats)
{
    if (!pf || !assoc || !assoc_stride || !stats) return SLAM_ERR_INVALID_ARG;
    if (!pf->assoc_tab) return SLAM_ERR_NOT_READY;   // slam_pf_assoc_set never switched association on
    *assoc = pf->assoc_tab;
    *assoc_stride = pf->Lp;
    *stats = pf->assoc_stats;
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

int slam_pf_sight_device_view(slam_pf* pf, const float** table, int32_t* bins, const int32_t** spared)
{
    if (!pf || !table || !bins || !spared) return SLAM_ERR_INVALID_ARG;
    if (!pf->sight_spared) return SLAM_ERR_NOT_READY;   // slam_pf_prune_sight_set never switched line of sight on
    *table = pf->e->sight_buf.as<float>();
    *bins = pf->sight_bins;
    *spared = pf->sight_spared;
    return SLAM_OK;
}

int slam_pf_fov_device_view(slam_pf* pf, float bounds[2], const int32_t** outside)
{
    if (!pf || !bounds || !outside) return SLAM_ERR_INVALID_ARG;
    if (!pf->fov_outside) return SLAM_ERR_NOT_READY;   // slam_pf_prune_fov_set never switched the field of view on
    bounds[0] = pf->fov_on ? pf->fov_lo : 0.0f;        // (off: everything is in view)
    bounds[1] = pf->fov_on ? pf->fov_hi : 4.0f;
    *outside = pf->fov_outside;
    return SLAM_OK;
}

int slam_pf_merge_device_view(slam_pf* pf, const int32_t** stats)
{
    if (!pf || !stats) return SLAM_ERR_INVALID_ARG;
    if (!pf->merge_stats) return SLAM_ERR_NOT_READY;   // slam_pf_merge_set never switched merging on
    *stats = pf->merge_stats;
    return SLAM_OK;
}

int slam_pf_assoc_weight_device_view(slam_pf* pf, const int32_t** missed, const float** terms)
{
    if (!pf || !missed || !terms) return SLAM_ERR_INVALID_ARG;
    if (!pf->assoc_weight_missed) return SLAM_ERR_NOT_READY;   // slam_pf_assoc_weight_set never switched it on
    *missed = pf->prune_on ? pf->assoc_weight_missed : nullptr;
    *terms = pf->assoc_weight_terms;
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
}  // extern "C"
