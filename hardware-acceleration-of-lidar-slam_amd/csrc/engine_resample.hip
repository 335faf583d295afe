// engine_resample.hip — the resample side of a particle-filter frame behind the C ABI: log-weights, quantise + scan, offspring
// and ancestors with the ESS gate, the comb offset, the sharded plan / pack / unpack stages, arg-max and the gathers.

#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include "engine_internal.h"

using namespace slam;

namespace {

// host-side Philox4x32-10 for the comb offset
void philox_host(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

}  // namespace

int slam_engine_bmax_ready(slam_engine* e)
{
    if (e->bmax_buf.cap < sizeof(float) * (size_t)logweight_scratch_floats()) {   // block maxima + a ticket word kept at zero
        SLAM_HIP_TRY(e, e->bmax_buf.ensure(sizeof(float) * (size_t)logweight_scratch_floats()));
        SLAM_HIP_TRY(e, hipMemsetAsync(e->bmax_buf.p, 0, e->bmax_buf.cap, e->stream));
    }
    return SLAM_OK;
}

int slam_engine_spread_result(slam_engine* e, const slam::PoseMean& mean, const long long m[slam::kPoseMoments], float pose[3],
                              float cov[6], float* heading_r)
{
    if (m[kPoseMomentsFlag] != 0) {
        snprintf(e->err, sizeof e->err, "pose spread: %lld particles lie 2048 m or more from the mean in x or y (or are not numbers)",
                 m[kPoseMomentsFlag]);
        return SLAM_ERR_INVALID_ARG;
    }
    if (!cov_from_moment_sums(m, cov)) {
        snprintf(e->err, sizeof e->err, "pose spread: the weights of the population sum to %lld", m[kPoseMomentsD]);
        return SLAM_ERR_INVALID_ARG;
    }
    for (int k = 0; k < 3; ++k) pose[k] = mean.pose[k];
    *heading_r = heading_length(mean);
    return SLAM_OK;
}

extern "C" {

static int logweight_common(slam_engine* e, const float* d_score, const float* d_loglik, float score_gain, int n,
                            float* d_logw, float* d_max, const CovArgs* cov = nullptr, int cov_bound = 0)
{
    if (n <= 0 || !d_logw) return SLAM_ERR_INVALID_ARG;
    if (int rc = slam_engine_bmax_ready(e)) return rc;
    const ProfScope prof(e, SLAM_PROF_WEIGHTS);
    // with a resample gate: the weights of a frame that did not resample carry into this one (device-side decision)
    const bool carry = e->gate_frac_q16 != 0 && e->carry_n == n;
    SLAM_HIP_TRY(e, launch_logweight(e->stream, d_score, d_loglik, score_gain, n, d_logw, e->bmax_buf.as<float>(), d_max,
                                     carry ? e->carry_buf.as<float>() : nullptr, carry ? e->gate_buf.as<int32_t>() : nullptr, cov, cov_bound));
    e->bmax_count = logweight_scratch_elems(n);
    e->bmax_n = n;
    return SLAM_OK;
}

int slam_logweight_dev(slam_engine* e, const float* d_score, const float* d_loglik, float score_gain, int n,
                       float* d_logw, float* d_max)
{
    SLAM_ENTER(e);
    return logweight_common(e, d_score, d_loglik, score_gain, n, d_logw, d_max);
}

int slam_logweight_ekf_dev(slam_engine* e, const float* d_score, float score_gain, int n, float* d_logw, float* d_max)
{
    SLAM_ENTER(e);
    if (e->ll_n != n) return SLAM_ERR_NOT_READY;   // needs slam_ekf_update_dev(…, n, …) on this engine first
    return logweight_common(e, d_score, e->ll_buf.as<float>(), score_gain, n, d_logw, d_max);
}

// the session's form: d_loglik == nullptr -> the log-likelihoods the last landmark update left in the engine (use_ekf) or none;
// cov: a split session's covariance classes are brought up to date by workgroups of the same launch
int slam_logweight_cov_dev(slam_engine* e, const float* d_score, bool use_ekf, float score_gain, int n, float* d_logw, float* d_max,
                           const CovArgs* cov, int cov_bound)
{
    SLAM_ENTER(e);
    if (use_ekf && e->ll_n != n) return SLAM_ERR_NOT_READY;
    return logweight_common(e, d_score, use_ekf ? e->ll_buf.as<float>() : nullptr, score_gain, n, d_logw, d_max, cov, cov_bound);
}

static int quantise_scan_common(slam_engine* e, const float* d_logw, const float* d_max, int n, uint64_t* d_sum, const CovArgs* cov,
                                int cov_bound)
{
    if (n <= 0 || !d_logw) return SLAM_ERR_INVALID_ARG;
    if (!d_max && e->bmax_n != n) return SLAM_ERR_NOT_READY;   // needs the maxima of slam_logweight_dev(n)
    const size_t ntiles = (size_t)scan_tile_count(n);
    SLAM_HIP_TRY(e, e->scan_state.ensure(sizeof(uint64_t) * ((size_t)n + 3 * ntiles + 1)));
    uint64_t* cdf = e->scan_state.as<uint64_t>();
    uint64_t* tiles = cdf + n;   // tile_total | tile_s16 | tile_q16
    float* carry = nullptr;
    if (e->gate_frac_q16 != 0) {
        SLAM_HIP_TRY(e, e->carry_buf.ensure(sizeof(float) * (size_t)n));
        carry = e->carry_buf.as<float>();
    }
    const ProfScope prof(e, SLAM_PROF_SCAN);
    SLAM_HIP_TRY(e, launch_quantise_scan(e->stream, d_logw, d_max, e->bmax_buf.as<float>(), e->bmax_count, n, cdf, tiles, d_sum,
                                         carry, tiles + ntiles, tiles + 2 * ntiles, e->gate_buf.as<unsigned int>() + kGateTicketWord, cov,
                                         cov_bound));
    e->scan_n = n;
    e->carry_n = carry ? n : -1;
    return SLAM_OK;
}

int slam_quantise_scan_dev(slam_engine* e, const float* d_logw, const float* d_max, int n, uint64_t* d_sum)
{
    SLAM_ENTER(e);
    return quantise_scan_common(e, d_logw, d_max, n, d_sum, nullptr, 0);
}

int slam_quantise_scan_cov_dev(slam_engine* e, const float* d_logw, int n, const CovArgs* cov, int cov_bound)
{
    SLAM_ENTER(e);
    if (e->gate_frac_q16 != 0) return SLAM_ERR_INVALID_ARG;   // (the rider exists for the ungated scan alone)
    return quantise_scan_common(e, d_logw, nullptr, n, nullptr, cov, cov_bound);
}

int slam_offspring_from_scan_dev(slam_engine* e, int n, const uint64_t* d_base, const uint64_t* d_total, uint64_t seed,
                                 uint32_t frame, int64_t n_total, int32_t* d_first)
{
    SLAM_ENTER(e);
    if (n <= 0 || n_total < n || n_total > 0x7fffffff || !d_first) return SLAM_ERR_INVALID_ARG;
    if (e->scan_n != n) return SLAM_ERR_NOT_READY;
    const uint64_t* cdf = e->scan_state.as<uint64_t>();
    // (a shard of a larger population: base and total come from the caller, so does the gate — not applied here)
    SLAM_HIP_TRY(e, launch_offspring_from_scan(e->stream, cdf, cdf + n, n, d_base, d_total, nullptr, 0, 1, seed, frame, n_total,
                                               d_first));
    return SLAM_OK;
}

int slam_ancestors_from_scan_dev(slam_engine* e, int n, uint64_t seed, uint32_t frame, int32_t* d_anc)
{
    return slam_ancestors_survivors_dev(e, n, seed, frame, d_anc, nullptr);
}

int slam_ancestors_survivors_dev(slam_engine* e, int n, uint64_t seed, uint32_t frame, int32_t* d_anc, const SurvivorOut* survivors)
{
    SLAM_ENTER(e);
    if (n <= 0 || !d_anc || (survivors && !ancestors_from_scan_fits(n))) return SLAM_ERR_INVALID_ARG;
    if (e->scan_n != n) return SLAM_ERR_NOT_READY;
    const uint64_t* cdf = e->scan_state.as<uint64_t>();
    const uint32_t frac = e->carry_n == n ? e->gate_frac_q16 : 0;   // the gate needs the sums of a gated quantise_scan
    const GateOut gate = frac ? e->gate_next() : GateOut();
    const ProfScope prof(e, SLAM_PROF_ANCESTORS);
    if (ancestors_from_scan_fits(n)) {
        // the distinct-ancestor count only steers the EKF's kernel choice: made only for populations that have maps
        SLAM_HIP_TRY(e, launch_ancestors_from_scan(e->stream, cdf, cdf + n, n, seed, frame, d_anc, frac, gate,
                                                   e->ll_n == n ? e->heads_out() : HeadsOut(), survivors ? *survivors : SurvivorOut()));
        return SLAM_OK;
    }
    // more tiles than the one-launch form keeps in LDS: the two-launch form through a scratch `first` array
    SLAM_HIP_TRY(e, e->first_buf.ensure(sizeof(int32_t) * (size_t)n));
    int32_t* first = e->first_buf.as<int32_t>();
    SLAM_HIP_TRY(e, launch_offspring_from_scan(e->stream, cdf, cdf + n, n, nullptr, nullptr, nullptr, 0, 1, seed, frame, n, first,
                                               frac, gate));
    SLAM_HIP_TRY(e, launch_ancestors(e->stream, first, n, 0, n, d_anc));
    return SLAM_OK;
}

int slam_offspring_from_scan_sharded_dev(slam_engine* e, int n, const uint64_t* d_shard_totals, int rank, int world,
                                         uint64_t seed, uint32_t frame, int64_t n_total, int32_t* d_first)
{
    SLAM_ENTER(e);
    if (n <= 0 || world < 1 || world > kMaxRanks || rank < 0 || rank >= world || n_total != (int64_t)n * world ||
        n_total > 0x7fffffff || !d_shard_totals || !d_first)
        return SLAM_ERR_INVALID_ARG;
    if (e->scan_n != n) return SLAM_ERR_NOT_READY;
    const uint64_t* cdf = e->scan_state.as<uint64_t>();
    const uint32_t frac = e->carry_n == n ? e->gate_frac_q16 : 0;
    const ProfScope prof(e, SLAM_PROF_ANCESTORS);
    SLAM_HIP_TRY(e, launch_offspring_from_scan(e->stream, cdf, cdf + n, n, nullptr, nullptr, d_shard_totals, rank, world, seed,
                                               frame, n_total, d_first, frac, frac ? e->gate_next() : GateOut()));
    return SLAM_OK;
}

int slam_resample_gate_set(slam_engine* e, float ess_frac)
{
    SLAM_ENTER(e);
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    e->gate_frac_q16 = ess_frac > 0.0f && ess_frac < 1.0f ? (uint32_t)lrintf(ess_frac * 65536.0f) : 0u;
    e->carry_n = -1;
    e->h_gate[0] = 1;
    const int32_t one = 1;   // nothing is carried into the next frame
    SLAM_HIP_TRY(e, hipMemcpy(e->gate_buf.p, &one, sizeof one, hipMemcpyHostToDevice));
    return SLAM_OK;
}

int slam_resample_happened_host(slam_engine* e, int* resampled)
{
    SLAM_ENTER(e);
    if (!resampled) return SLAM_ERR_INVALID_ARG;
    *resampled = 1;
    if (e->gate_frac_q16 == 0 || e->gate_seq == 0) return SLAM_OK;   // no gate (or no gated stage yet): every frame resamples
    volatile uint32_t* h_seq = reinterpret_cast<volatile uint32_t*>(e->h_gate + 1);
    const uint32_t seq = e->gate_seq;
    if (int rc = slam_engine_wait_flag(e, e->comm, h_seq, seq, "resample gate flag")) return rc;   // sharded: the verdict sits behind collectives
    *resampled = e->h_gate[0] != 0;
    return SLAM_OK;
}

int slam_resample_heads_host(slam_engine* e, int32_t* heads, int32_t* n)
{
    SLAM_ENTER(e);
    if (!heads || !n) return SLAM_ERR_INVALID_ARG;
    *heads = e->h_heads[0];   // mapped host memory, read as the engine's own heuristic reads it: no wait
    *n = e->h_heads[1];
    return SLAM_OK;
}

int slam_quantise_weights_dev(slam_engine* e, const float* d_logw, const float* d_max, int n, uint64_t* d_wq,
                              uint64_t* d_sum)
{
    SLAM_ENTER(e);
    if (n < 0 || !d_max || !d_sum || (n > 0 && (!d_logw || !d_wq))) return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_quantise_weights(e->stream, d_logw, d_max, n, d_wq, d_sum));
    return SLAM_OK;
}

int slam_prefix_sum_dev(slam_engine* e, const uint64_t* d_wq, int n, uint64_t* d_cdf)
{
    SLAM_ENTER(e);
    if (n < 0 || (n > 0 && (!d_wq || !d_cdf))) return SLAM_ERR_INVALID_ARG;
    if (n == 0) return SLAM_OK;
    SLAM_HIP_TRY(e, e->scratch.ensure(sizeof(uint64_t) * (size_t)prefix_sum_scratch_elems(n)));
    SLAM_HIP_TRY(e, launch_prefix_sum(e->stream, d_wq, n, d_cdf, e->scratch.as<uint64_t>()));
    return SLAM_OK;
}

int slam_offspring_offsets_dev(slam_engine* e, const uint64_t* d_cdf, int n, const uint64_t* d_base,
                               const uint64_t* d_total, uint64_t seed, uint32_t frame, int64_t n_total,
                               int32_t* d_first)
{
    SLAM_ENTER(e);
    if (n < 0 || n_total < n || n_total > 0x7fffffff || !d_total || (n > 0 && (!d_cdf || !d_first)))
        return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_offspring_offsets(e->stream, d_cdf, n, d_base, d_total, seed, frame, n_total, d_first));
    return SLAM_OK;
}

int slam_ancestors_dev(slam_engine* e, const int32_t* d_first_all, int64_t n_total, int64_t slot0, int nslots,
                       int32_t* d_anc)
{
    SLAM_ENTER(e);
    if (nslots < 0 || n_total <= 0 || slot0 < 0 || slot0 + nslots > n_total || !d_first_all || (nslots > 0 && !d_anc))
        return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_ancestors(e->stream, d_first_all, n_total, slot0, nslots, d_anc));
    return SLAM_OK;
}

uint64_t slam_comb_offset(uint64_t seed, uint32_t frame, uint64_t total)
{
    uint32_t c[4] = { 0u, 0u, frame, 1u /* resample stream */ };
    philox_host(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t r64 = (uint64_t)c[0] | ((uint64_t)c[1] << 32);
    return (uint64_t)(((unsigned __int128)r64 * total) >> 64);
}

static bool make_plan(MigratePlan& plan, const int64_t* lo, const int32_t* cnt, int world)
{
    if (world < 1 || world > kMaxRanks || !lo || !cnt) return false;
    plan.world = world;
    int64_t off = 0;
    for (int q = 0; q < world; ++q) {
        if (cnt[q] < 0 || lo[q] < 0) return false;
        plan.lo[q] = lo[q];
        plan.off[q] = (int32_t)off;
        off += cnt[q];
        if (off > 0x7fffffff) return false;
    }
    plan.off[world] = (int32_t)off;
    return true;
}

int slam_ancestors_sharded_dev(slam_engine* e, const int32_t* d_first_all, int64_t n_total, int n_local, int rank,
                               int world, int32_t* d_src, int32_t* d_plan, int32_t* d_pose_idx)
{
    SLAM_ENTER(e);
    if (n_local <= 0 || world < 1 || world > kMaxRanks || rank < 0 || rank >= world ||
        n_total != (int64_t)n_local * world || !d_first_all || !d_src || !d_plan ||
        (d_pose_idx && 3 * n_total > 0x7fffffff))
        return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, e->shard_buf.ensure(sizeof(int32_t) * (size_t)shard_scan_words(n_local)));
    const uint32_t seq = ++e->plan_seq;
    const ProfScope prof(e, SLAM_PROF_PLAN);
    SLAM_HIP_TRY(e, launch_ancestors_sharded(e->stream, d_first_all, n_total, n_local, rank, world, e->shard_buf.as<int32_t>(),
                                             d_plan, d_src, d_pose_idx, e->d_hplan,
                                             reinterpret_cast<uint32_t*>(e->d_hplan + SLAM_PLAN_WORDS(kMaxRanks)), seq, e->exch_cap,
                                             e->d_hheads));
    e->shard_n = n_local;   // what slam_migrate_pack_dev will read
    e->plan_world = world;
    return SLAM_OK;
}

int slam_exchange_set_capacity(slam_engine* e, int recv_capacity)
{
    SLAM_ENTER(e);
    e->exch_cap = recv_capacity > 0 ? recv_capacity : 0x7fffffff;
    return SLAM_OK;
}

int slam_exchange_plan_host(slam_engine* e, int world, int32_t* plan)
{
    SLAM_ENTER(e);
    if (!plan || world < 1 || world > kMaxRanks) return SLAM_ERR_INVALID_ARG;
    if (e->plan_seq == 0 || e->plan_world != world) return SLAM_ERR_NOT_READY;
    volatile uint32_t* h_flag = reinterpret_cast<volatile uint32_t*>(e->h_plan + SLAM_PLAN_WORDS(kMaxRanks));
    const uint32_t seq = e->plan_seq;
    // with a communicator the plan kernel sits behind this frame's collectives: the wait polls it, bounded in time
    if (int rc = slam_engine_wait_flag(e, e->comm, h_flag, seq, "exchange plan flag")) return rc;
    memcpy(plan, e->h_plan, sizeof(int32_t) * (size_t)SLAM_PLAN_WORDS(world));
    return SLAM_OK;
}

int slam_migrate_pack_dev(slam_engine* e, int n_local, int rank, int world, const int32_t* plan, const float* d_pose,
                          int64_t pose_ld, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                          float* d_out)
{
    return slam_migrate_pack_paged(e, n_local, rank, world, plan, d_pose, pose_ld, d_map, row_stride, plane_stride, nlandmarks,
                                   d_out, nullptr, 0, nullptr, nullptr, nullptr);
}

// d_pt != nullptr: d_map is a page pool and the particles' landmarks sit behind page tables of nb entries (pf_session_store.hip)
int slam_migrate_pack_paged(slam_engine* e, int n_local, int rank, int world, const int32_t* plan, const float* d_pose,
                            int64_t pose_ld, const float* d_map, int64_t row_stride, int plane_stride, int nlandmarks,
                            float* d_out, const int32_t* d_pt, int nb, const float* d_split_cov, const int32_t* d_split_cls,
                            const slam::PageGeom* geom)
{
    SLAM_ENTER(e);
    if (n_local <= 0 || world < 1 || world > kMaxRanks || rank < 0 || rank >= world || !plan || nlandmarks < 0 ||
        !d_pose || (nlandmarks > 0 && (!d_map || plane_stride < nlandmarks || row_stride < (d_split_cls ? 2 : 5) * (int64_t)plane_stride)) ||
        (d_split_cls && !d_split_cov) || (d_split_cls && d_pt && !geom))
        return SLAM_ERR_INVALID_ARG;
    if (e->shard_n != n_local) return SLAM_ERR_NOT_READY;   // needs slam_ancestors_sharded_dev(n_local) of this frame
    MigratePlan mp;
    int64_t base[kMaxRanks];
    for (int q = 0; q < world; ++q) base[q] = plan[1 + 2 * world + q];
    if (!make_plan(mp, base, plan + 1, world) || plan[1 + rank] != 0) return SLAM_ERR_INVALID_ARG;
    if (mp.off[world] > 0 && !d_out) return SLAM_ERR_INVALID_ARG;
    const ProfScope prof(e, SLAM_PROF_PACK);
    SLAM_HIP_TRY(e, launch_migrate_pack(e->stream, e->shard_buf.as<int32_t>(), n_local, mp, d_pose, pose_ld, d_map, row_stride,
                                        plane_stride, nlandmarks, d_out, d_pt, nb, d_split_cov, d_split_cls, geom ? *geom : PageGeom()));
    return SLAM_OK;
}

int slam_migrate_unpack_dev(slam_engine* e, const float* d_in, int world, const int32_t* recv_cnt, int n_local,
                            float* d_pose, int64_t pose_ld, float* d_map, int64_t row_stride, int plane_stride,
                            int nlandmarks)
{
    SLAM_ENTER(e);
    MigratePlan plan;
    int64_t zeros[kMaxRanks] = { 0 };
    if (!make_plan(plan, zeros, recv_cnt, world) || n_local <= 0 || nlandmarks < 0 || !d_pose ||
        (nlandmarks > 0 && (!d_map || plane_stride < nlandmarks || row_stride < 5 * (int64_t)plane_stride)))
        return SLAM_ERR_INVALID_ARG;
    if (plan.off[world] > 0 && !d_in) return SLAM_ERR_INVALID_ARG;
    if ((int64_t)n_local + plan.off[world] > pose_ld) return SLAM_ERR_CAPACITY;   // pose_ld = particle capacity
    const ProfScope prof(e, SLAM_PROF_UNPACK);
    SLAM_HIP_TRY(e, launch_migrate_unpack(e->stream, d_in, plan, n_local, d_pose, pose_ld, d_map, row_stride, plane_stride,
                                          nlandmarks));
    return SLAM_OK;
}

int slam_argmax_dev(slam_engine* e, const float* d_values, int n, int32_t* d_index, float* d_value)
{
    SLAM_ENTER(e);
    if (n <= 0 || !d_values || !d_index || !d_value) return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_argmax(e->stream, d_values, n, d_index, d_value));
    return SLAM_OK;
}

int slam_pose_spread_dev(slam_engine* e, const float* d_x, const float* d_y, const float* d_theta, const int32_t* d_idx,
                         const float* d_carry, int n, float ref_theta, float pose[3], float cov[6], float* heading_r)
{
    SLAM_ENTER(e);
    if (n <= 0 || !d_x || !d_y || !d_theta || !pose || !cov || !heading_r) return SLAM_ERR_INVALID_ARG;
    // 8-byte words: the sums' accumulators and ticket | the moments' accumulators and ticket | what either launch hands over
    constexpr size_t kSumsAt = 0, kMomentsAt = kPoseSumsWeighted + 1, kOutAt = kMomentsAt + kPoseMoments + 1, kWords = kOutAt + kPoseMoments;
    if (!e->spread_buf.p) {
        SLAM_HIP_TRY(e, e->spread_buf.ensure(kWords * 8));
        SLAM_HIP_TRY(e, hipMemsetAsync(e->spread_buf.p, 0, kWords * 8, e->stream));
    }
    unsigned long long* w = e->spread_buf.as<unsigned long long>();
    long long* d_out = reinterpret_cast<long long*>(w + kOutAt);
    long long h[kPoseMoments];
    auto sums = [&](const float* carry) -> int {
        SLAM_HIP_TRY(e, launch_pose_sums(e->stream, d_x, d_y, d_theta, d_idx, n, ref_theta, w + kSumsAt,
                                         reinterpret_cast<unsigned int*>(w + kSumsAt + kPoseSumsWeighted), d_out, nullptr, nullptr, 0, carry));
        SLAM_HIP_TRY(e, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
        return SLAM_OK;
    };
    if (d_carry)
        if (int rc = sums(d_carry)) return rc;
    const bool weighted = d_carry && h[kPoseSumsWeighted - 1] > 0;   // (no weight at all: the plain form, as slam_pf_mean)
    if (!weighted)
        if (int rc = sums(nullptr)) return rc;
    const PoseMean m = weighted ? mean_from_weighted_sums(h, ref_theta) : mean_from_plain_sums(h, n, ref_theta);
    SLAM_HIP_TRY(e, launch_pose_moments(e->stream, d_x, d_y, d_theta, d_idx, n, m.pose, w + kMomentsAt,
                                        reinterpret_cast<unsigned int*>(w + kMomentsAt + kPoseMoments), d_out, nullptr, nullptr, 0,
                                        weighted ? d_carry : nullptr));
    SLAM_HIP_TRY(e, hipMemcpyAsync(h, d_out, sizeof h, hipMemcpyDeviceToHost, e->stream));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return slam_engine_spread_result(e, m, h, pose, cov, heading_r);
}

int slam_gather_f32_dev(slam_engine* e, const float* d_src, const int32_t* d_idx, int n, float* d_dst)
{
    SLAM_ENTER(e);
    if (n < 0 || (n > 0 && (!d_src || !d_idx || !d_dst)) || d_src == d_dst) return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_gather_f32(e->stream, d_src, d_idx, n, d_dst));
    return SLAM_OK;
}

int slam_gather_map_dev(slam_engine* e, const float* d_map_in, float* d_map_out, int64_t in_row_stride,
                        int64_t out_row_stride, int in_plane_stride, int out_plane_stride, int nlandmarks,
                        const int32_t* d_idx, int n)
{
    SLAM_ENTER(e);
    if (n < 0 || nlandmarks < 0 || in_plane_stride < nlandmarks || out_plane_stride < nlandmarks ||
        in_row_stride < 5 * (int64_t)in_plane_stride || out_row_stride < 5 * (int64_t)out_plane_stride ||
        (n > 0 && nlandmarks > 0 && (!d_map_in || !d_map_out || !d_idx)) || d_map_in == d_map_out)
        return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, launch_gather_map(e->stream, d_map_in, d_map_out, in_row_stride, out_row_stride, in_plane_stride,
                                      out_plane_stride, nlandmarks, d_idx, n));
    return SLAM_OK;
}

}  // extern "C"
