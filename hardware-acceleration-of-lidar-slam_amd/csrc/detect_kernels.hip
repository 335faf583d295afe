// detect_kernels.hip — the landmark detector (no counterpart in the reference; specification: tests/_detect_spec.py, DESIGN.md
// section 7): the engine's current scan, P <= SLAM_MAX_BEAMS sensor-frame points in scan order, becomes the frame's DETECTIONS —
// the centroids of the short, narrow, unoccluded runs of points between two range jumps — where slam_associate_dev looks for them.
//
// ONE WORKGROUP, one launch: a latency kernel on the frame's critical path, sized by the scan (a thread owns up to four points
// b = k * T + tid; T = 64 .. 1024 threads), not a throughput kernel.
//   1. the scan goes to LDS (at most 32 KB);
//   2. break_b = !(gap to the predecessor <= jump^2): a wavefront's 64 flags are one ballot = one 64-bit word of the break mask
//      (the points of a wavefront in round k are the 64 consecutive points of word (k * T + wave * 64) / 64);
//   3. the owner of a break is the lane of its segment: the segment's end comes from the mask (the first set bit behind f, looked
//      for in at most max_points + 1 positions — three words), then the tests and the sequential centroid sum (m <= 64 LDS reads);
//   4. the accepted flags are a second mask of the same shape, so "ascending f" is the order of its bits: a detection's place is
//      the number of set bits in front of it (an exclusive prefix over the 64 word popcounts by wavefront 0, plus the popcount of
//      the lanes in front) — no atomics, and nothing depends on the order in which lanes or wavefronts arrive;
//   5. zx[64] | zy[64] (0 from ndet on), the stats and {ndet, sequence} in mapped host memory: plain vector stores, the sequence
//      word released last.
// THE FIT (kFit, a compile-time policy: the instantiation without it is the kernel as it was; specification:
// tests/_detect_fit_spec.py): a pole of known radius rho.  Directly behind the centroid sum the owning lane walks its segment's
// m <= 64 LDS points once more for their spread s2 about the centroid; s2 <= rho^2 + tol^2 or the segment is no pole (the shape
// test: a third mask of the same shape, only counted), and the detection is the point sqrt(rho^2 - s2) behind the centroid on
// its line of sight — the circle's centre.
// THE NOISE MODEL (kNoise, a second compile-time policy; specification: tests/_detect_noise_spec.py): the owning lane gives the
// point that passed its range test its covariance Q = a u u^T + b v v^T (det_noise: one rounded operation per line of the spec);
// r2 == 0 or a Q that fails the rule of ekf_aniso_cov_ok is no detection (a fourth mask, only counted), in front of the cap.

#include "kernels.h"

namespace slam {

namespace {

typedef unsigned long long u64;

constexpr int kDetRounds = 4;                       // points per thread
constexpr int kDetMaxThreads = SLAM_MAX_BEAMS / kDetRounds;
constexpr int kDetWords = SLAM_MAX_BEAMS / 64;
static_assert(kDetMaxThreads == 1024 && kDetWords == 64, "one mask word per lane of wavefront 0");

// the smallest p in [lo, hi) whose bit is set, -1: none (hi <= 64 * kDetWords)
__device__ __forceinline__ int first_set(const u64* mask, int lo, int hi)
{
    if (lo >= hi) return -1;
    const int w0 = lo >> 6, w1 = (hi - 1) >> 6;
    for (int w = w0; w <= w1; ++w) {
        u64 m = mask[w];
        if (w == w0) m &= ~0ull << (lo & 63);
        if (w == w1 && (hi & 63)) m &= (1ull << (hi & 63)) - 1ull;
        if (m) return (w << 6) + __ffsll(m) - 1;
    }
    return -1;
}

struct DetScan {
    const float *x, *y;   // LDS
    int P, wrap;
};

// squared gap of point b to its predecessor (cyclic with wrap; point 0 without: +inf) — four separately rounded operations
__device__ __forceinline__ float det_gap(const DetScan& s, int b)
{
    if (b == 0 && !s.wrap) return __uint_as_float(0x7f800000u);
    const int p = b > 0 ? b - 1 : s.P - 1;
    const float dx = s.x[b] - s.x[p], dy = s.y[b] - s.y[p];
    const float dx2 = dx * dx, dy2 = dy * dy;
    return dx2 + dy2;
}

__device__ __forceinline__ float det_r2(const DetScan& s, int b)
{
    const float xx = s.x[b] * s.x[b], yy = s.y[b] * s.y[b];
    return xx + yy;
}

// Q of the detection (zx, zy), r2 = zx * zx + zy * zy as its range test formed it; false: no detection
__device__ __forceinline__ bool det_noise(const DetectNoiseArgs& nz, float zx, float zy, float r2, float& qxx, float& qxy, float& qyy)
{
    if (!(r2 > 0.0f)) return false;
    const float rho = sqrtf(r2);
    const float ux = zx / rho, uy = zy / rho;
    const float a = nz.range_var;
    const float t = nz.bearing_var * r2;
    const float b = t + nz.lateral_var;
    const float uxx = ux * ux, uyy = uy * uy, uxy = ux * uy;
    const float x0 = a * uxx, x1 = b * uyy;
    qxx = x0 + x1;
    const float d = a - b;
    qxy = d * uxy;
    const float y0 = a * uyy, y1 = b * uxx;
    qyy = y0 + y1;
    const float d0 = qxx * qyy, d1 = qxy * qxy;
    EkfAnisoCov q{ qxx, qxy, qyy, d0 - d1 };
    return ekf_aniso_cov_ok(q);
}

// the segment that starts at break f: accepted -> its centroid, with kFit the centre fitted to it (shape: the shape test rejected it)
template <bool kFit>
__device__ __forceinline__ bool det_segment(const DetScan& s, const DetectArgs& a, const u64* brk, int f, float& zx, float& zy,
                                            bool& shape, float& r2)
{
    const int P = s.P, span = a.max_points + 1;   // an implementation may stop counting at max_points + 1
    int q = first_set(brk, f + 1, min(f + span + 1, P)), m = -1;
    if (q >= 0) m = q - f;
    else if (s.wrap && f + span >= P) {           // ... through P - 1 into 0, as far as f itself (the only break: the whole scan)
        q = first_set(brk, 0, min(f + span + 1 - P, f + 1));
        if (q >= 0) m = q + P - f;
    }
    // without wrap a segment that holds point 0 or point P - 1 is cut by the field of view (no break behind f: it holds P - 1)
    if (m < a.min_points || m > a.max_points || (!s.wrap && f == 0)) return false;
    int e = f + m - 1;
    e = e >= P ? e - P : e;
    const int p = f > 0 ? f - 1 : P - 1;
    const float wx = s.x[e] - s.x[f], wy = s.y[e] - s.y[f];
    const float wx2 = wx * wx, wy2 = wy * wy;
    if (!(wx2 + wy2 <= a.width2)) return false;
    if (det_gap(s, f) <= a.guard2 && det_r2(s, p) < det_r2(s, f)) return false;   // occluded on the left
    if (det_gap(s, q) <= a.guard2 && det_r2(s, q) < det_r2(s, e)) return false;   // ... on the right
    float sx = s.x[f], sy = s.y[f];
    for (int j = 1, i = f; j < m; ++j) {
        i = i + 1 == P ? 0 : i + 1;
        sx = sx + s.x[i];
        sy = sy + s.y[i];
    }
    const float fm = (float)m;
    zx = sx / fm;   // IEEE division (-fno-fast-math)
    zy = sy / fm;
    const float zxx = zx * zx, zyy = zy * zy;
    if constexpr (!kFit) {
        r2 = zxx + zyy;
        return r2 <= a.range2;   // NaN and inf fail: what comes out is finite
    } else {
        const float c2 = zxx + zyy;
        if (!(c2 <= a.range2)) return false;   // ... so everything that enters the fit is finite
        const float cx = zx, cy = zy;
        float q = 0.0f;
        for (int j = 0, i = f; j < m; ++j) {   // the same walk: the spread about the centroid, in segment order
            const float du = s.x[i] - cx, dv = s.y[i] - cy;
            const float du2 = du * du, dv2 = dv * dv;
            q = q + (du2 + dv2);
            i = i + 1 == P ? 0 : i + 1;
        }
        const float s2 = q / fm;
        if (!(s2 <= a.lim) || !(c2 > 0.0f)) {   // not round enough for a pole / the centroid on the sensor: no line of sight
            shape = true;
            return false;
        }
        float t = a.rho2 - s2;
        t = t > 0.0f ? t : 0.0f;
        const float d = sqrtf(t), n = sqrtf(c2);   // correctly rounded (hipcc's default, like the divisions)
        const float ux = cx / n, uy = cy / n;
        const float ox = d * ux, oy = d * uy;
        zx = cx + ox;
        zy = cy + oy;
        const float fxx = zx * zx, fyy = zy * zy;
        r2 = fxx + fyy;
        return r2 <= a.range2;
    }
}

template <bool kFit, bool kNoise>
__device__ __forceinline__ void detect_scan_body(const DetectArgs& a, const DetectNoiseArgs& nz)
{
    __shared__ float s_x[SLAM_MAX_BEAMS], s_y[SLAM_MAX_BEAMS];
    __shared__ u64 s_brk[kDetWords], s_acc[kDetWords], s_shp[kFit ? kDetWords : 1], s_nz[kNoise ? kDetWords : 1];
    __shared__ int s_pre[kDetWords], s_tot[kNoise ? 4 : kFit ? 3 : 2];
    const int T = (int)blockDim.x, tid = (int)threadIdx.x, lane = tid & 63;
    const int P = a.nbeams, nwords = (kDetRounds * T) >> 6;   // the words the ballots below write (kDetRounds * T >= P)
    DetScan s;
    s.x = s_x;
    s.y = s_y;
    s.P = P;
    s.wrap = a.wrap;

#pragma unroll
    for (int k = 0; k < kDetRounds; ++k) {
        const int b = k * T + tid;
        if (b < P) {
            s_x[b] = a.bx[b];
            s_y[b] = a.by[b];
        }
    }
    __syncthreads();

    unsigned mine = 0;   // bit k: my point of round k is a break
#pragma unroll
    for (int k = 0; k < kDetRounds; ++k) {
        const int b = k * T + tid;
        const bool brk = b < P && !(det_gap(s, b) <= a.jump2);   // a NaN breaks
        const u64 word = __ballot(brk);
        if (lane == 0) s_brk[b >> 6] = word;
        mine |= brk ? 1u << k : 0u;
    }
    __syncthreads();

    float zx[kDetRounds], zy[kDetRounds];
    float qxx[kNoise ? kDetRounds : 1], qxy[kNoise ? kDetRounds : 1], qyy[kNoise ? kDetRounds : 1];
    unsigned kept = 0;
#pragma unroll
    for (int k = 0; k < kDetRounds; ++k) {
        const int b = k * T + tid;
        zx[k] = 0.0f;
        zy[k] = 0.0f;
        bool acc = false, shape = false;
        float r2 = 0.0f;
        if ((mine >> k) & 1u) acc = det_segment<kFit>(s, a, s_brk, b, zx[k], zy[k], shape, r2);
        if constexpr (kNoise) {   // the fourth mask: passed its range test, dropped by the noise rule
            qxx[k] = qxy[k] = qyy[k] = 0.0f;
            const bool ok = acc && det_noise(nz, zx[k], zy[k], r2, qxx[k], qxy[k], qyy[k]);
            const u64 dropped = __ballot(acc && !ok);
            if (lane == 0) s_nz[b >> 6] = dropped;
            acc = ok;
        }
        const u64 word = __ballot(acc);
        if (lane == 0) s_acc[b >> 6] = word;
        if constexpr (kFit) {   // the third mask: rejected by the shape test
            const u64 round = __ballot(shape);
            if (lane == 0) s_shp[b >> 6] = round;
        }
        kept |= acc ? 1u << k : 0u;
    }
    __syncthreads();

    if (tid < 64) {   // wavefront 0, lane w: word w
        const int c = tid < nwords ? __popcll(s_acc[tid]) : 0;
        int segs = tid < nwords ? __popcll(s_brk[tid]) : 0;
        int shp = 0;
        if constexpr (kFit) shp = tid < nwords ? __popcll(s_shp[tid]) : 0;
        int nzd = 0;
        if constexpr (kNoise) nzd = tid < nwords ? __popcll(s_nz[tid]) : 0;
        int inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64), other = __shfl_xor(segs, d, 64);
            inc += lane >= d ? up : 0;
            segs += other;
            if constexpr (kFit) shp += __shfl_xor(shp, d, 64);
            if constexpr (kNoise) nzd += __shfl_xor(nzd, d, 64);
        }
        s_pre[tid] = inc - c;
        if (tid == 63) s_tot[0] = inc;
        if (tid == 0) s_tot[1] = segs;
        if constexpr (kFit)
            if (tid == 0) s_tot[2] = shp;
        if constexpr (kNoise)
            if (tid == 0) s_tot[3] = nzd;
    }
    __syncthreads();

    const int accepted = s_tot[0], written = min(accepted, (int)SLAM_MAX_DETECTIONS);
#pragma unroll
    for (int k = 0; k < kDetRounds; ++k) {
        if (!((kept >> k) & 1u)) continue;
        const int w = (k * T + tid) >> 6;
        const int rank = s_pre[w] + __popcll(s_acc[w] & ((1ull << lane) - 1ull));
        if (rank < SLAM_MAX_DETECTIONS) {
            a.det[rank] = zx[k];
            a.det[SLAM_MAX_DETECTIONS + rank] = zy[k];
            if constexpr (kNoise) {
                nz.cov[rank] = qxx[k];
                nz.cov[SLAM_MAX_DETECTIONS + rank] = qxy[k];
                nz.cov[2 * SLAM_MAX_DETECTIONS + rank] = qyy[k];
            }
        }
    }
    if (tid < SLAM_MAX_DETECTIONS && tid >= written) {
        a.det[tid] = 0.0f;
        a.det[SLAM_MAX_DETECTIONS + tid] = 0.0f;
        if constexpr (kNoise) {
            nz.cov[tid] = 0.0f;
            nz.cov[SLAM_MAX_DETECTIONS + tid] = 0.0f;
            nz.cov[2 * SLAM_MAX_DETECTIONS + tid] = 0.0f;
        }
    }
    if (tid == 0) {
        if (a.stats) {
            a.stats[0] = s_tot[1];
            a.stats[1] = accepted;
            a.stats[2] = written;
            if constexpr (kFit) a.stats[3] = s_tot[2];
            else a.stats[3] = 0;
            if constexpr (kNoise) {
                a.stats[4] = s_tot[3];
                a.stats[5] = 0;
            }
        }
        a.h_out[0] = written;
        __threadfence_system();
        __hip_atomic_store(reinterpret_cast<uint32_t*>(a.h_out + 1), a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

template <bool kFit> __global__ __launch_bounds__(kDetMaxThreads) void detect_scan_kernel(DetectArgs a)
{
    detect_scan_body<kFit, false>(a, DetectNoiseArgs{});
}

// ... with the noise model: Q beside every detection, the noise rule in front of the cap, six stats words
template <bool kFit> __global__ __launch_bounds__(kDetMaxThreads) void detect_scan_noise_kernel(DetectArgs a, DetectNoiseArgs nz)
{
    detect_scan_body<kFit, true>(a, nz);
}

}  // namespace

hipError_t launch_detect_scan(hipStream_t stream, const DetectArgs& a, const EventPair* ev, const DetectNoiseArgs* noise)
{
    if (a.nbeams < 0 || a.nbeams > SLAM_MAX_BEAMS || a.min_points < 1 || a.max_points > SLAM_DETECT_MAX_POINTS ||
        a.min_points > a.max_points || !a.det || !a.h_out || (a.nbeams > 0 && (!a.bx || !a.by)) || (a.fit != 0 && a.fit != 1))
        return hipErrorInvalidValue;   // what the LDS arrays and the mask search are sized by
    int threads = ((a.nbeams + kDetRounds - 1) / kDetRounds + 63) & ~63;
    threads = threads < 64 ? 64 : threads;
    if (ev) (void)hipEventRecord(ev->start, stream);
    if (noise && !noise->cov) return hipErrorInvalidValue;
    if (noise && a.fit) detect_scan_noise_kernel<true><<<1, threads, 0, stream>>>(a, *noise);
    else if (noise) detect_scan_noise_kernel<false><<<1, threads, 0, stream>>>(a, *noise);
    else if (a.fit) detect_scan_kernel<true><<<1, threads, 0, stream>>>(a);
    else detect_scan_kernel<false><<<1, threads, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace slam
