// estimate_host.h — the host arithmetic behind slam_pf_mean and slam_pf_spread, written once for the session (pf_session_read.hip)
// and the engine-level call (engine_resample.hip: slam_pose_spread_dev): from the integer sums pose_sums_kernel and
// pose_moments_kernel leave to the floats of include/slam_hip.h.  Restated in Python integers by tests/_estimate_spec.py and
// tests/_spread_spec.py.
#pragma once

#include <math.h>
#include <stdint.h>

#include "kernels.h"

namespace slam {

// the mean and what of its sums the spread wants: Qs, Qc = trunc(sum S / D), trunc(sum C / D)
struct PoseMean {
    float pose[3];
    long long qs, qc;
};

// the plain mean from {sum X, sum Y, sum S, sum C} over n_total particles
inline PoseMean mean_from_plain_sums(const long long s[kPoseSumsPlain], int64_t n_total, float ref_theta)
{
    PoseMean m;
    const double nt = (double)n_total;
    m.pose[0] = (float)((double)s[0] / 4294967296.0 / nt);
    m.pose[1] = (float)((double)s[1] / 4294967296.0 / nt);
    m.pose[2] = (float)((double)ref_theta + atan2((double)s[2], (double)s[3]));
    m.qs = s[2] / n_total;   // C's division truncates
    m.qc = s[3] / n_total;
    return m;
}

// the weighted mean from the nine limb sums; needs w[8] = sum w16 > 0
inline PoseMean mean_from_weighted_sums(const long long w[kPoseSumsWeighted], float ref_theta)
{
    PoseMean m;
    long long q[4];
    for (int k = 0; k < 4; ++k)   // trunc(sum w16 V / sum w16): C's division truncates
        q[k] = (long long)(((__int128)w[2 * k] * 2097152 + w[2 * k + 1]) / w[8]);
    m.pose[0] = (float)((double)q[0] / 4294967296.0);
    m.pose[1] = (float)((double)q[1] / 4294967296.0);
    m.pose[2] = (float)((double)ref_theta + atan2((double)q[2], (double)q[3]));
    m.qs = q[2];
    m.qc = q[3];
    return m;
}

// length of the mean heading vector
inline float heading_length(const PoseMean& m) { return (float)(hypot((double)m.qs, (double)m.qc) / 1073741824.0); }

// cov[6] from pose_moments_kernel's sums: the three limbs of each of the six sums joined in 128 bits, divided (towards zero) by
// D = m[kPoseMomentsD], out of 2^-40 fixed point.  false: D <= 0
inline bool cov_from_moment_sums(const long long m[kPoseMoments], float cov[6])
{
    const long long d = m[kPoseMomentsD];
    if (d <= 0) return false;
    for (int k = 0; k < 6; ++k) {
        const __int128 total = ((__int128)m[3 * k + 2] * 2097152 + m[3 * k + 1]) * 2097152 + m[3 * k];   // limbs 2^21 apart
        cov[k] = (float)((double)(long long)(total / d) / 1099511627776.0);
    }
    return true;
}

}  // namespace slam
