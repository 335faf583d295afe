// engine_reseed.hip — reseeding the cloud from what the lidar sees behind the C ABI (reseed_kernels.hip): one launch over the
// engine's current detections and a known map as it was given; a chosen fraction of the slots becomes pose proposals, the rest
// take the pending resample.  The two counts come back by a copy (slam_pose_reseed_dev) or, for the session, through mapped host
// memory (slam_engine_pose_reseed).  The same for proposals from detection PAIRS (reseed_pair_kernels.hip; four counts):
// slam_pose_reseed_pairs_dev, slam_engine_pose_reseed_pairs.

#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>

#include "engine_internal.h"

using namespace slam;

namespace {

// do the n floats at a and the n floats at b share an address?
bool overlap(const float* a, const float* b, int n)
{
    const uintptr_t ua = reinterpret_cast<uintptr_t>(a), ub = reinterpret_cast<uintptr_t>(b), bytes = sizeof(float) * (uintptr_t)n;
    return ua < ub + bytes && ub < ua + bytes;
}

// what both reseeds refuse, in this order; the detections are resolved
int check_args(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x_in, const float* d_y_in,
               const float* d_th_in, const int32_t* d_anc, float* d_x_out, float* d_y_out, float* d_th_out, int n, float fraction,
               bool counts_have_a_home)
{
    if (n <= 0 || nlandmarks <= 0 || plane_stride < nlandmarks || !(fraction > 0.0f && fraction <= 1.0f) || !d_map || !d_x_in || !d_y_in ||   // (NaN fails every comparison)
        !d_th_in || !d_x_out || !d_y_out || !d_th_out || !counts_have_a_home)
        return SLAM_ERR_INVALID_ARG;
    // in place — every out array IS its in array — exactly when no gather is pending; any other overlap of in and out is refused
    const float* in[3] = { d_x_in, d_y_in, d_th_in };
    float* out[3] = { d_x_out, d_y_out, d_th_out };
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b)
            if (overlap(in[a], out[b], n) && !(a == b && !d_anc && in[a] == out[b])) {
                snprintf(e->err, sizeof e->err, "reseed: in and out overlap (in place, out == in, is for d_anc == NULL only)");
                return SLAM_ERR_INVALID_ARG;
            }
    if (e->ndet < 0) return SLAM_ERR_NOT_READY;
    return SLAM_OK;
}

}  // namespace

int slam_engine_pose_reseed(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x_in, const float* d_y_in,
                            const float* d_th_in, const int32_t* d_anc, float* d_x_out, float* d_y_out, float* d_th_out, int n,
                            int64_t first_id, uint64_t seed, uint32_t frame, float fraction, uint8_t* d_flag,
                            const slam_reseed_mapped* mapped, int32_t counts[2], bool* launched)
{
    SLAM_ENTER(e);
    if (launched) *launched = false;
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (int rc = check_args(e, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n, fraction,
                            mapped || counts))
        return rc;
    if (e->ndet == 0) {   // nothing to propose from: nothing is written
        if (counts) counts[0] = counts[1] = 0;
        return SLAM_OK;
    }
    // 4-byte words: the two accumulators, the ticket, a spare | the two counts
    constexpr size_t kOutAt = 4, kWords = 6;
    if (!e->reseed_buf.p) {
        SLAM_HIP_TRY(e, e->reseed_buf.ensure(kWords * 4));
        SLAM_HIP_TRY(e, hipMemsetAsync(e->reseed_buf.p, 0, kWords * 4, e->stream));
    }
    ReseedArgs a;
    a.map = d_map;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x_in = d_x_in;
    a.y_in = d_y_in;
    a.th_in = d_th_in;
    a.anc = d_anc;
    a.x_out = d_x_out;
    a.y_out = d_y_out;
    a.th_out = d_th_out;
    a.n = n;
    a.det_zx = e->d_det_zx;
    a.det_zy = e->d_det_zy;
    a.ndet = e->ndet;
    a.first_id = (uint64_t)first_id;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.frame = frame;
    a.thr = (uint64_t)floor((double)fraction * 4294967296.0);   // fraction == 1: 2^32, every slot
    a.flag = d_flag;
    a.acc = e->reseed_buf.as<unsigned int>();
    a.out = e->reseed_buf.as<int32_t>() + kOutAt;
    a.h_out = mapped ? mapped->d_hout : nullptr;
    a.h_seq = mapped ? mapped->d_hseq : nullptr;
    a.seq = mapped ? mapped->seq : 0u;
    SLAM_HIP_TRY(e, launch_pose_reseed(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->reseed_launches++;
    if (launched) *launched = true;
    if (!mapped) {
        SLAM_HIP_TRY(e, hipMemcpyAsync(counts, a.out, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
    return SLAM_OK;
}

int slam_engine_pose_reseed_pairs(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x_in,
                                  const float* d_y_in, const float* d_th_in, const int32_t* d_anc, float* d_x_out, float* d_y_out,
                                  float* d_th_out, int n, int64_t first_id, uint64_t seed, uint32_t frame, float fraction, float tol,
                                  float min_sep, uint8_t* d_flag, const slam_reseed_mapped* mapped, int32_t counts[4], bool* launched)
{
    SLAM_ENTER(e);
    if (launched) *launched = false;
    if (int rc = slam_engine_resolve_detections(e)) return rc;
    if (!(tol >= 0.0f) || !(min_sep > tol) || !isfinite(min_sep) || nlandmarks == 1) {   // (NaN fails every comparison; tol < min_sep is finite)
        snprintf(e->err, sizeof e->err, "reseed from pairs: 0 <= tol < min_sep, both finite, and a map of two landmarks or more");
        return SLAM_ERR_INVALID_ARG;
    }
    if (int rc = check_args(e, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n, fraction,
                            mapped || counts))
        return rc;
    if (e->ndet < 2) {   // no pair to propose from: nothing is written
        if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
        return SLAM_OK;
    }
    // 4-byte words: the four accumulators, the ticket, three spare | the four counts
    constexpr size_t kOutAt = 8, kWords = 12;
    if (!e->reseed_pair_buf.p) {
        SLAM_HIP_TRY(e, e->reseed_pair_buf.ensure(kWords * 4));
        SLAM_HIP_TRY(e, hipMemsetAsync(e->reseed_pair_buf.p, 0, kWords * 4, e->stream));
    }
    ReseedPairArgs a;
    a.map = d_map;
    a.plane_stride = plane_stride;
    a.nlandmarks = nlandmarks;
    a.x_in = d_x_in;
    a.y_in = d_y_in;
    a.th_in = d_th_in;
    a.anc = d_anc;
    a.x_out = d_x_out;
    a.y_out = d_y_out;
    a.th_out = d_th_out;
    a.n = n;
    a.det_zx = e->d_det_zx;
    a.det_zy = e->d_det_zy;
    a.ndet = e->ndet;
    a.first_id = (uint64_t)first_id;
    a.key0 = (uint32_t)seed;
    a.key1 = (uint32_t)(seed >> 32);
    a.frame = frame;
    a.thr = (uint64_t)floor((double)fraction * 4294967296.0);   // fraction == 1: 2^32, every slot
    a.tol = tol;
    a.min_sep2 = min_sep * min_sep;   // (one rounding: this unit is compiled without contraction, and nothing is added)
    a.flag = d_flag;
    a.acc = e->reseed_pair_buf.as<unsigned int>();
    a.out = e->reseed_pair_buf.as<int32_t>() + kOutAt;
    a.h_out = mapped ? mapped->d_hout : nullptr;
    a.h_seq = mapped ? mapped->d_hseq : nullptr;
    a.seq = mapped ? mapped->seq : 0u;
    SLAM_HIP_TRY(e, launch_pose_reseed_pairs(e->stream, a, e->prof_next(SLAM_PROF_PAGES)));
    e->reseed_pair_launches++;
    if (launched) *launched = true;
    if (!mapped) {
        SLAM_HIP_TRY(e, hipMemcpyAsync(counts, a.out, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    }
    return SLAM_OK;
}

extern "C" {

int slam_pose_reseed_pairs_dev(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x_in,
                               const float* d_y_in, const float* d_th_in, const int32_t* d_anc, float* d_x_out, float* d_y_out,
                               float* d_th_out, int n, int64_t first_id, uint64_t seed, uint32_t frame, float fraction, float tol,
                               float min_sep, uint8_t* d_flag, int32_t counts[4])
{
    return slam_engine_pose_reseed_pairs(e, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n,
                                         first_id, seed, frame, fraction, tol, min_sep, d_flag, nullptr, counts, nullptr);
}

int slam_pose_reseed_pairs_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->reseed_pair_launches;
    return SLAM_OK;
}

int slam_pose_reseed_dev(slam_engine* e, const float* d_map, int plane_stride, int nlandmarks, const float* d_x_in, const float* d_y_in,
                         const float* d_th_in, const int32_t* d_anc, float* d_x_out, float* d_y_out, float* d_th_out, int n,
                         int64_t first_id, uint64_t seed, uint32_t frame, float fraction, uint8_t* d_flag, int32_t counts[2])
{
    return slam_engine_pose_reseed(e, d_map, plane_stride, nlandmarks, d_x_in, d_y_in, d_th_in, d_anc, d_x_out, d_y_out, d_th_out, n,
                                   first_id, seed, frame, fraction, d_flag, nullptr, counts, nullptr);
}

int slam_pose_reseed_count(slam_engine* e, int64_t* launches)
{
    SLAM_ENTER(e);
    if (!launches) return SLAM_ERR_INVALID_ARG;
    *launches = e->reseed_launches;
    return SLAM_OK;
}

}  // extern "C"
