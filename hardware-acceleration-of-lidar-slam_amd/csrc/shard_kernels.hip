// shard_kernels.hip — the resample of a sharded (multi-GPU) session: the gather index of a rank's slots, the exchange plan
// with duplicates removed, pack / unpack of the migrating particles.
//
// No reference counterpart: the specification is DESIGN.md + oracle/slam_oracle_pf.c, matched bit for bit.

#include "block_reduce.h"
#include "resample_common.h"

namespace slam {

namespace {

// ------------------------------------------------------------------ multi-GPU resample: sharded gather index + migration
// Slots of rank r are [r*n, (r+1)*n).  The particles of rank s fill the slot range [A_s, B_s) with
// A_s = first_all[s*n], B_s = A_(s+1) (B of the last rank = n_total) because `first` is non-decreasing.
// So what rank r receives from rank s is ONE contiguous run of its slots, and everything below follows
// from the world+1 boundary values — no host-computed plan is needed for the index kernel.
__device__ __forceinline__ int64_t first_or_total(const int32_t* __restrict__ first_all, int64_t idx, int64_t n_total)
{
    return idx < n_total ? (int64_t)first_all[idx] : n_total;
}

// (last_with_first_le: resample_common.h)
// ---- exchange with duplicates removed.  After a resample many slots share one ancestor; a remote ancestor's row
// is sent ONCE per destination rank, however many of that rank's slots descend from it.  Both sides derive the
// same order from first_all alone:
//   receiver r: D(j) = number of "heads" among its slots up to j (a slot is a head when it is the first of r's
//               slots with that ancestor); the rows received from rank s land in the staging tail in ancestor
//               order, and slot j finds its row at  n + roff[s] + D(j) - D(first slot served by s);
//   sender  s:  P(a) = number of its particles up to a that have any offspring; the rows for rank d are the
//               particles with offspring in d's slot range, in order: the q-th is the first a with
//               P(a) = P(first ancestor of the run) + q.
// Both counts are prefix sums over n elements (two-level: 2048-element tiles, then the tile totals).
constexpr int kShardTile = kScanTile;                  // elements per workgroup in the flag scan: the tile of the CDF's scan
constexpr int kShardItems = kScanItems;                // per thread

// global ancestor of each of my slots: one thread per slot
__global__ __launch_bounds__(kBlock) void shard_search_kernel(const int32_t* __restrict__ first_all, int64_t n_total, int n,
                                                              int rank, int32_t* __restrict__ gsrc)
{
    const int jl = blockIdx.x * kBlock + threadIdx.x;
    if (jl < n) gsrc[jl] = (int32_t)last_with_first_le(first_all, n_total, (int64_t)rank * n + jl);
}

// y = 0: head flags of my slots;  y = 1: "has offspring" flags of my particles
__global__ __launch_bounds__(kBlock) void shard_flag_scan_kernel(const int32_t* __restrict__ first_all, int64_t n_total,
                                                                 int n, int rank, const int32_t* __restrict__ gsrc,
                                                                 int32_t* __restrict__ pfx, int32_t* __restrict__ btot,
                                                                 int ntiles)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int y = blockIdx.y;
    const int64_t my_lo = (int64_t)rank * n;
    const int base = blockIdx.x * kShardTile + threadIdx.x * kShardItems;
    int32_t f[kShardItems];
    int32_t run = 0;
    if (y == 0) {
        // the ancestors were found by shard_search_kernel, one thread per slot (a thread doing its kShardItems
        // searches itself is 136 dependent L2 round trips: 20 us for this kernel instead of 5 + 5)
#pragma unroll
        for (int k = 0; k < kShardItems; ++k) {
            const int idx = base + k;
            int32_t flag = 0;
            if (idx < n) {
                const int64_t g = gsrc[idx];
                flag = (idx == 0 || (int64_t)first_all[g] == my_lo + idx) ? 1 : 0;
            }
            run += flag;
            f[k] = run;
        }
    } else {
#pragma unroll
        for (int k = 0; k < kShardItems; ++k) {
            const int idx = base + k;
            int32_t flag = 0;
            if (idx < n) {
                const int64_t j = my_lo + idx;
                flag = first_or_total(first_all, j + 1, n_total) > (int64_t)first_all[j] ? 1 : 0;
            }
            run += flag;
            f[k] = run;   // inclusive within the thread
        }
    }
    // exclusive offset of this thread inside the tile
    int32_t total;
    const int32_t excl = block_inclusive_scan<int32_t, false>(run, s_wave, total) - run;
#pragma unroll
    for (int k = 0; k < kShardItems; ++k)
        if (base + k < n) pfx[(int64_t)y * n + base + k] = excl + f[k];
    if (threadIdx.x == kBlock - 1) btot[y * ntiles + blockIdx.x] = total;
}

__device__ __forceinline__ int32_t shard_prefix(const int32_t* __restrict__ pfx, const int32_t* __restrict__ boff, int y,
                                                int n, int ntiles, int idx)   // inclusive count up to idx
{
    return pfx[(int64_t)y * n + idx] + boff[y * ntiles + idx / kShardTile];
}

// One workgroup: tile totals -> exclusive tile offsets (in place), then the per-peer plan.
// plan (int32, device, visible to the host): [0] anything moves (same on every rank) | send_cnt[world] |
// recv_cnt[world] | send_base[world];   rplan (device only): roff[world] | rbase[world]
__global__ __launch_bounds__(kBlock) void shard_plan_kernel(const int32_t* __restrict__ first_all, int64_t n_total, int n,
                                                            int rank, int world, const int32_t* __restrict__ pfx,
                                                            int32_t* __restrict__ boff, int ntiles,
                                                            int32_t* __restrict__ plan, int32_t* __restrict__ rplan,
                                                            int32_t* __restrict__ host_plan,
                                                            uint32_t* __restrict__ host_flag, uint32_t seq, int recv_cap,
                                                            int32_t* __restrict__ host_heads)
{
    __shared__ int32_t s_part[kBlock];
    for (int y = 0; y < 2; ++y) {   // exclusive scan of the tile totals, kBlock-sized chunks with a running carry
        int32_t carry = 0;
        for (int c0 = 0; c0 < ntiles; c0 += kBlock) {
            const int t = c0 + threadIdx.x;
            const int32_t v = t < ntiles ? boff[y * ntiles + t] : 0;
            s_part[threadIdx.x] = v;
            __syncthreads();
            for (int o = 1; o < kBlock; o <<= 1) {
                const int32_t add = (int)threadIdx.x >= o ? s_part[threadIdx.x - o] : 0;
                __syncthreads();
                s_part[threadIdx.x] += add;
                __syncthreads();
            }
            if (t < ntiles) boff[y * ntiles + t] = carry + s_part[threadIdx.x] - v;
            carry += s_part[kBlock - 1];
            __syncthreads();
        }
    }
    __threadfence_block();
    __syncthreads();
    // one thread per peer (their binary searches run side by side: one thread doing all peers in turn is ~10 us of
    // dependent L2 round trips per peer), then thread 0 strings the receive offsets together
    __shared__ int32_t s_scnt[kMaxRanks], s_rcnt[kMaxRanks], s_sbase[kMaxRanks], s_rbase[kMaxRanks], s_any[kMaxRanks];
    const int64_t my_lo = (int64_t)rank * n, my_hi = my_lo + n;
    if ((int)threadIdx.x < world) {
        const int q = threadIdx.x;
        const int64_t a_me = first_or_total(first_all, my_lo, n_total), b_me = first_or_total(first_all, my_hi, n_total);
        const int64_t aq = first_or_total(first_all, (int64_t)q * n, n_total);
        const int64_t bq = first_or_total(first_all, (int64_t)(q + 1) * n, n_total);
        s_any[q] = (q > 0 && aq != (int64_t)q * n) ? 1 : 0;   // a run boundary off a rank boundary: somebody exchanges
        {   // could rank q's staging area overflow?  Decided from the boundary values alone, so that EVERY rank reaches
            // the same verdict about EVERY rank: the slots of q with an ancestor on another rank bound what q receives
            const int64_t q0 = (int64_t)q * n, q1 = q0 + n;
            const int64_t l = aq > q0 ? aq : q0, h = bq < q1 ? bq : q1;
            const int64_t local_slots = h > l ? h - l : 0;
            if ((int64_t)n - local_slots > (int64_t)recv_cap) s_any[q] |= 2;
        }
        // what I receive from q: my slots [lo, hi) descend from q's particles
        int64_t lo = aq > my_lo ? aq : my_lo, hi = bq < my_hi ? bq : my_hi;
        int32_t rcnt = 0, rbase = 0;
        if (q != rank && hi > lo) {
            rbase = shard_prefix(pfx, boff, 0, n, ntiles, (int)(lo - my_lo));
            rcnt = shard_prefix(pfx, boff, 0, n, ntiles, (int)(hi - 1 - my_lo)) - rbase + 1;
        }
        // what I send to q: q's slots [lo, hi) descend from my particles
        const int64_t q_lo = (int64_t)q * n, q_hi = q_lo + n;
        lo = a_me > q_lo ? a_me : q_lo;
        hi = b_me < q_hi ? b_me : q_hi;
        int32_t scnt = 0, sbase = 0;
        if (q != rank && hi > lo) {
            const int a_lo = (int)(last_with_first_le(first_all, n_total, lo) - my_lo);
            const int a_hi = (int)(last_with_first_le(first_all, n_total, hi - 1) - my_lo);
            sbase = shard_prefix(pfx, boff, 1, n, ntiles, a_lo);
            scnt = shard_prefix(pfx, boff, 1, n, ntiles, a_hi) - sbase + 1;
        }
        s_scnt[q] = scnt;
        s_rcnt[q] = rcnt;
        s_sbase[q] = sbase;
        s_rbase[q] = rbase;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int32_t anything = 0, roff = 0;
    for (int q = 0; q < world; ++q) {
        anything |= s_any[q];
        rplan[q] = roff;
        rplan[world + q] = s_rbase[q];
        roff += s_rcnt[q];
        plan[1 + q] = s_scnt[q];
        plan[1 + world + q] = s_rcnt[q];
        plan[1 + 2 * world + q] = s_sbase[q];
        if (host_plan) {
            host_plan[1 + q] = s_scnt[q];
            host_plan[1 + world + q] = s_rcnt[q];
            host_plan[1 + 2 * world + q] = s_sbase[q];
        }
    }
    if (host_heads) {   // distinct ancestors among my slots = heads (feedback for the choice of the EKF form)
        host_heads[0] = shard_prefix(pfx, boff, 0, n, ntiles, n - 1);
        host_heads[1] = n;
    }
    plan[0] = anything;   // bit 0: somebody exchanges rows; bit 1: some rank's staging area might not hold them
    if (host_plan) {   // zero-copy delivery: the host polls the flag instead of a device-to-host copy + stream sync
        host_plan[0] = anything;
        __threadfence_system();
        __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// src[jl]: where slot r*n + jl finds its ancestor — a local particle index, or n + its row in the staging tail
__global__ __launch_bounds__(kBlock) void ancestors_sharded_kernel(const int32_t* __restrict__ gsrc,
                                                                   const int32_t* __restrict__ pfx,
                                                                   const int32_t* __restrict__ boff, int ntiles,
                                                                   const int32_t* __restrict__ rplan, int n, int rank,
                                                                   int world, int32_t* __restrict__ src,
                                                                   int32_t* __restrict__ pose_idx)
{
    const int jl = blockIdx.x * kBlock + threadIdx.x;
    if (jl >= n) return;
    const int32_t g = gsrc[jl];
    const int owner = g / n;
    // where the ancestor's pose sits in an all-gather of the ranks' [x | y | theta] blocks (3 n floats per rank)
    if (pose_idx) pose_idx[jl] = owner * 3 * n + (g - owner * n);
    src[jl] = owner == rank ? g - rank * n
                            : n + rplan[owner] + (shard_prefix(pfx, boff, 0, n, ntiles, jl) - rplan[world + owner]);
}

// Pack what the other ranks need from me into one buffer: block d (for rank d) is cnt_d records of 3 + 5L floats
// — x, y, theta, then the five map planes (L values each) — one record per DISTINCT particle of mine with
// offspring among d's slots, in particle order.  One workgroup per record, one launch for every destination.
__global__ __launch_bounds__(kBlock) void migrate_pack_kernel(const int32_t* __restrict__ pfx,
                                                              const int32_t* __restrict__ boff, int ntiles, int n,
                                                              MigratePlan plan, const float* __restrict__ pose,
                                                              int64_t pose_ld, const float* __restrict__ map,
                                                              int64_t row_stride, int plane_stride, int nlandmarks,
                                                              float* __restrict__ out, const int32_t* __restrict__ pt,
                                                              int nb, const float* __restrict__ split_cov,
                                                              const int32_t* __restrict__ split_cls, PageGeom geom)
{
    const int p = blockIdx.x;
    int d = 0;
    while (p >= plan.off[d + 1]) ++d;
    const int32_t target = (int32_t)plan.lo[d] + (p - plan.off[d]);   // P value of the wanted particle
    int lo = 0, hi = n - 1;                                            // first a with P(a) >= target
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (shard_prefix(pfx, boff, 1, n, ntiles, mid) >= target) hi = mid; else lo = mid + 1;
    }
    const int loc = lo;
    float* __restrict__ rec = out + (int64_t)(3 + 5 * nlandmarks) * p;
    if (threadIdx.x < 3) rec[threadIdx.x] = pose[threadIdx.x * pose_ld + loc];
    if (pt && split_cls) {   // split pages: the means behind the page table (pages of two planes, kernels.h: PageGeom), the
        const int32_t* __restrict__ tab = pt + (int64_t)loc * nb;   // covariance planes in the class's rows
        const float* __restrict__ crow = split_cov + (int64_t)split_cls[loc] * 3 * plane_stride;
        for (int pl = 0; pl < 5; ++pl)
            for (int l = threadIdx.x; l < nlandmarks; l += kBlock) {
                const int64_t page = tab[l / kPageLandmarks];
                rec[3 + pl * nlandmarks + l] =
                    pl < 2 ? map[page * (2 * kPageLandmarks) + (page >= geom.half_pages ? geom.gap : 0) + pl * kPageLandmarks + l % kPageLandmarks]
                           : crow[(pl - 2) * plane_stride + l];
            }
        return;
    }
    if (pt) {   // paged maps: `map` is the page pool, the particle's landmarks sit behind its page table (paged_kernels.hip)
        const int32_t* __restrict__ tab = pt + (int64_t)loc * nb;
        for (int pl = 0; pl < 5; ++pl)
            for (int l = threadIdx.x; l < nlandmarks; l += kBlock)
                rec[3 + pl * nlandmarks + l] = map[(int64_t)tab[l / kPageLandmarks] * (5 * kPageLandmarks) + pl * kPageLandmarks +
                                                   l % kPageLandmarks];
        return;
    }
    const float* __restrict__ row = map + (int64_t)loc * row_stride;
    if (split_cls) {   // split layout: `map` holds the means (two planes), the covariance planes are the class's (split_kernels.hip)
        const float* __restrict__ crow = split_cov + (int64_t)split_cls[loc] * 3 * plane_stride;
        for (int pl = 0; pl < 5; ++pl)
            for (int l = threadIdx.x; l < nlandmarks; l += kBlock)
                rec[3 + pl * nlandmarks + l] = pl < 2 ? row[pl * plane_stride + l] : crow[(pl - 2) * plane_stride + l];
        return;
    }
    for (int pl = 0; pl < 5; ++pl)
        for (int l = threadIdx.x; l < nlandmarks; l += kBlock) rec[3 + pl * nlandmarks + l] = row[pl * plane_stride + l];
}

// Unpack the received records into the staging tail behind the n local particles (position = running index
// over sources in rank order, matching ancestors_sharded_kernel).
__global__ __launch_bounds__(kBlock) void migrate_unpack_kernel(const float* __restrict__ in, int total, int n,
                                                                float* __restrict__ pose, int64_t pose_ld,
                                                                float* __restrict__ map, int64_t row_stride,
                                                                int plane_stride, int nlandmarks)
{
    const int p = blockIdx.x;
    if (p >= total) return;
    const float* __restrict__ rec = in + (int64_t)(3 + 5 * nlandmarks) * p;
    if (threadIdx.x < 3) pose[threadIdx.x * pose_ld + n + p] = rec[threadIdx.x];
    float* __restrict__ row = map + (int64_t)(n + p) * row_stride;
    for (int pl = 0; pl < 5; ++pl)
        for (int l = threadIdx.x; l < nlandmarks; l += kBlock) row[pl * plane_stride + l] = rec[3 + pl * nlandmarks + l];
}

}  // namespace

int shard_scan_words(int n) { const int t = (n + kShardTile - 1) / kShardTile; return 3 * n + 2 * t + 2 * kMaxRanks; }

// scratch (int32 words, shard_scan_words(n)): gsrc[n] | pfx[2][n] | boff[2][ntiles] | rplan[2*kMaxRanks]
hipError_t launch_ancestors_sharded(hipStream_t stream, const int32_t* first_all, int64_t n_total, int n, int rank,
                                    int world, int32_t* scratch, int32_t* plan, int32_t* src, int32_t* pose_idx,
                                    int32_t* host_plan, uint32_t* host_flag, uint32_t seq, int recv_cap,
                                    int32_t* host_heads)
{
    if (n <= 0) return hipSuccess;
    const int ntiles = (n + kShardTile - 1) / kShardTile;
    int32_t* gsrc = scratch;
    int32_t* pfx = gsrc + n;
    int32_t* boff = pfx + 2 * (int64_t)n;
    int32_t* rplan = boff + 2 * ntiles;
    shard_search_kernel<<<blocks_for(n), kBlock, 0, stream>>>(first_all, n_total, n, rank, gsrc);
    shard_flag_scan_kernel<<<dim3(ntiles, 2), kBlock, 0, stream>>>(first_all, n_total, n, rank, gsrc, pfx, boff, ntiles);
    shard_plan_kernel<<<1, kBlock, 0, stream>>>(first_all, n_total, n, rank, world, pfx, boff, ntiles, plan, rplan,
                                                host_plan, host_flag, seq, recv_cap, host_heads);
    ancestors_sharded_kernel<<<blocks_for(n), kBlock, 0, stream>>>(gsrc, pfx, boff, ntiles, rplan, n, rank, world, src,
                                                                   pose_idx);
    return hipGetLastError();
}

// plan.lo[d] = send_base[d] (the P value of the first particle sent to d), plan.off = running record offsets
hipError_t launch_migrate_pack(hipStream_t stream, const int32_t* scratch, int n, const MigratePlan& plan,
                               const float* pose, int64_t pose_ld, const float* map, int64_t row_stride,
                               int plane_stride, int nlandmarks, float* out, const int32_t* pt, int nb, const float* split_cov,
                               const int32_t* split_cls, const PageGeom& geom)
{
    const int total = plan.off[plan.world];
    if (total <= 0) return hipSuccess;
    const int ntiles = (n + kShardTile - 1) / kShardTile;
    const int32_t* pfx = scratch + n;
    const int32_t* boff = pfx + 2 * (int64_t)n;
    migrate_pack_kernel<<<total, kBlock, 0, stream>>>(pfx, boff, ntiles, n, plan, pose, pose_ld, map, row_stride,
                                                     plane_stride, nlandmarks, out, pt, nb, split_cov, split_cls, geom);
    return hipGetLastError();
}

hipError_t launch_migrate_unpack(hipStream_t stream, const float* in, const MigratePlan& plan, int n, float* pose,
                                 int64_t pose_ld, float* map, int64_t row_stride, int plane_stride, int nlandmarks)
{
    const int total = plan.off[plan.world];
    if (total <= 0) return hipSuccess;
    migrate_unpack_kernel<<<total, kBlock, 0, stream>>>(in, total, n, pose, pose_ld, map, row_stride, plane_stride,
                                                       nlandmarks);
    return hipGetLastError();
}

}  // namespace slam
