// pf_session_store.hip — the storage forms of a session's landmark maps (rows, pages, split, split pages; pf_session.h) and the
// moves between them: allocation and placement in the one store, SLAM_MAP_AUTO's conversions (auto_layout), the grow-only
// scratch buffers, and the survivor rows of a dense split frame (materialise, settle_means).

#include "pf_session.h"

namespace slam::session {

// ---- the landmark maps live in ONE allocation `store` of 2 x cap x 5 x Lp floats, seen either as two row buffers
// (map[0] = the first half, map[1] = the second) or as a pool of 2 x cap x nb pages (the same bytes: a page is 5 x 32 floats,
// a row nb of them).  The page tables, free list and stamps exist only for sessions that may be on pages.
bool alloc_store(slam_pf* pf)
{
    const size_t half = (size_t)pf->row_stride() * (size_t)pf->cap;   // floats
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
    const size_t half = (size_t)pf->row_stride() * (size_t)pf->cap, unit = (size_t)pf->Lp * (size_t)pf->cap;
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

// ---- scratch
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
static int conversion_scratch(slam_pf* pf, size_t floats)
{
    if (pf->conv_floats >= floats) return SLAM_OK;   // (an alloc + free per move would serialise the frame every time)
    if (int rc = replace_scratch(pf, (void**)&pf->conv_tmp, floats * 4, false)) return rc;
    pf->conv_floats = pf->conv_tmp ? floats : 0;
    if (!pf->conv_tmp) pf->auto_stuck = true;
    return SLAM_OK;
}

// ---- moves between the forms
// The rows a move takes along.  Sharded: when the exchange of the last frame has already been completed (a map getter between two
// frames does that), the pending gather index also names rows of the staging tail, n .. n + rows_received - 1: they move with the rest.
static int rows_to_convert(const slam_pf* pf)
{
    return pf->n + (pf->comm && pf->has_anc && !pf->exchange_pending ? pf->rows_received : 0);
}

// the current rows at `src` (dense, `stride` floats each) -> pages page_base + r * nb + b behind identity tables, so the pending
// gather index means the same thing afterwards: ONE kernel, stream-ordered, no allocation
static int rows_to_pages(slam_pf* pf, const float* src, int64_t stride, int page_base)
{
    pf->pt_cur = 0;
    SLAM_HIP_TRY(pf->e, launch_pages_from_rows(pf->e->stream, src, stride, pf->Lp, pf->L, rows_to_convert(pf), page_pool(pf), page_base));
    pf->paged = true;
    return SLAM_OK;
}

// rows -> pages while the session runs.  The current rows sit in one half of the store (before the pending gather); they are
// written as pages into the OTHER half, and the half they came from becomes free pages.
static int convert_to_pages(slam_pf* pf)
{
    const int mc = pf->map_cur;
    return rows_to_pages(pf, pf->map[mc], pf->row_stride(), (1 - mc) * pf->cap * pf->nb);
}

// pages -> dense rows of `stride` floats (5 planes off pages, 2 off split pages) at `dst`, the first buffer: the pages lie
// anywhere in the store, a row buffer is one contiguous part of it, so the rows are put together in a scratch buffer first (row r
// = the pages table row r names, again before the pending gather) and copied.  While it runs this takes half as much memory
// again; when that is not to be had the session stays on pages (pf->paged stays set).
static int pages_to_rows(slam_pf* pf, int64_t stride, float* dst)
{
    slam_engine* e = pf->e;
    const int nrows = rows_to_convert(pf);
    const size_t used = (size_t)stride * (size_t)nrows;
    if (int rc = conversion_scratch(pf, used)) return rc;
    if (!pf->conv_tmp) return SLAM_OK;
    // stream-ordered: pages -> scratch rows -> the first buffer (the scratch is read before anything else writes it)
    SLAM_HIP_TRY(e, launch_rows_from_pages(e->stream, page_pool(pf), nullptr, nrows, pf->conv_tmp, stride, pf->Lp, pf->L));
    SLAM_HIP_TRY(e, hipMemcpyAsync(dst, pf->conv_tmp, used * 4, hipMemcpyDeviceToDevice, e->stream));
    pf->paged = false;
    return SLAM_OK;
}

// pages -> rows, into the first half of the store
static int convert_to_rows(slam_pf* pf)
{
    if (int rc = pages_to_rows(pf, pf->row_stride(), pf->map[0])) return rc;
    if (!pf->paged) pf->map_cur = 0;
    return SLAM_OK;
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

// split -> split pages: the means of the current buffer become pages in the OTHER mean buffer (identity tables, shifted),
// the buffer they came from becomes free pages; classes and covariances stay where they are.  One stream-ordered launch.
int split_means_to_pages(slam_pf* pf)
{
    const float* dst = pf->mean[1 - pf->sp_cur];
    // (sharded: rows_to_convert takes the staging tail along when the exchange of the last frame has been completed already)
    return rows_to_pages(pf, pf->mean[pf->sp_cur], pf->mean_stride(), dst == split_pool(pf) ? 0 : pf->cap * pf->nb);
}

// split pages -> split: the pages lie anywhere in the two mean buffers, so the rows are put together in the scratch buffer of
// convert_to_rows first and copied into mean[0]; the classes of the current particles follow into cls[0]
static int convert_split_pages_to_split(slam_pf* pf)
{
    slam_engine* e = pf->e;
    if (int rc = pages_to_rows(pf, pf->mean_stride(), pf->mean[0])) return rc;
    if (pf->paged) return SLAM_OK;
    if (pf->sp_cur == 1)
        SLAM_HIP_TRY(e, hipMemcpyAsync(pf->cls[0], pf->cls[1], (size_t)rows_to_convert(pf) * 4, hipMemcpyDeviceToDevice, e->stream));
    pf->sp_cur = 0;
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
    const bool to_pages = !pf->paged && pf->votes_pages >= 3;
    if (!to_pages && !(pf->paged && pf->votes_rows >= 3)) return SLAM_OK;
    if (int rc = settle_means(pf)) return rc;   // a move reads every row
    if (int rc = to_pages ? (pf->split ? split_means_to_pages(pf) : convert_to_pages(pf))   // (split: the classes stay where they are)
                          : (pf->split ? convert_split_pages_to_split(pf) : convert_to_rows(pf)))
        return rc;
    if (pf->paged == to_pages) pf->conversions++;   // (a move off pages whose scratch was not to be had has not happened)
    return SLAM_OK;
}

// ---- survivor rows: the mean rows of the pending frame, from the inputs it started from (the same device functions as its front
// launch: the same bits) — for the particles the resample kept (filtered), or all of them.
int materialise(slam_pf* pf, bool filtered)
{
    const size_t sn = (size_t)pf->n;
    SplitIO sio{};
    sio.cov = pf->save_cov;
    sio.cov_stride = pf->cov_stride();
    sio.covx = pf->save_covx;
    sio.covx_stride = pf->mean_stride();
    sio.cls_in = pf->surv.cls_in;
    return slam_ekf_materialise_dev(pf->e, pf->surv.mean_in, pf->surv.mean_out, pf->mean_stride(), pf->Lp, pf->L, pf->obs_save,
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

}  // namespace slam::session
