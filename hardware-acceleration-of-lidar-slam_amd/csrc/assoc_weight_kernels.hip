// assoc_weight_kernels.hip — the weight of what a frame's association leaves unexplained (no counterpart in the reference;
// specification: tests/_assoc_weight_spec.py): the landmark update's log-likelihood sums one term per MATCHED
// pair, a log density in 1/m^2; a detection that started a landmark, one that was dropped and a landmark in view that took none
// contributed 0.  With three constants <= 0 — FastSLAM with unknown data association: the likelihood of a new feature, the clutter
// density, 1 - P_D — each of the three counts of a particle enters its log-likelihood in front of the weights.
//
// assoc_weight_kernel: one thread per particle, no atomics, no reduction.  It reads the association's stats row (created and
// dropped), the evidence stage's miss count (or none) and the log-likelihood, and does six separately rounded float32 operations
// in the specification's order; the counts are at most 64 and SLAM_MAX_OBS: exact in float32.  Traffic per particle: 20 B read,
// 8 B written — a launch that is all latency at every population a session has.

#include "kernels.h"

namespace slam {

namespace {

constexpr int kAssocWeightBlock = 256;

__global__ __launch_bounds__(kAssocWeightBlock) void assoc_weight_kernel(AssocWeightArgs a)
{
#pragma clang fp contract(off)
    const int i = (int)(blockIdx.x * kAssocWeightBlock + threadIdx.x);
    if (i >= a.n) return;
    const int32_t* st3 = a.stats + 3 * (size_t)i;
    const float created = (float)st3[1], dropped = (float)st3[2];
    const float missed = a.missed ? (float)a.missed[i] : 0.0f;
    float t = created * a.log_new;
    float u = dropped * a.log_clutter;
    t = t + u;
    u = missed * a.log_miss;
    t = t + u;
    a.loglik[i] = a.loglik[i] + t;
    if (a.terms) a.terms[i] = t;
}

}  // namespace

// finite and <= 0 (-0.0 is; NaN fails)
bool assoc_weight_const_ok(float v) { return v <= 0.0f && v >= -3.402823466e+38f; }

hipError_t launch_assoc_weight(hipStream_t stream, const AssocWeightArgs& a, const EventPair* ev)
{
    if (a.n <= 0) return hipSuccess;
    if (!a.stats || !a.loglik || !assoc_weight_const_ok(a.log_new) || !assoc_weight_const_ok(a.log_clutter) || !assoc_weight_const_ok(a.log_miss))
        return hipErrorInvalidValue;
    const int blocks = (a.n + kAssocWeightBlock - 1) / kAssocWeightBlock;
    if (ev) (void)hipEventRecord(ev->start, stream);
    assoc_weight_kernel<<<blocks, kAssocWeightBlock, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
