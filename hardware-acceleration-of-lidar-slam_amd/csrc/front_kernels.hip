// front_kernels.hip — the landmark update fused with the scorer into the front of a frame.
// ---- the FRONT of a single-GPU frame in one launch: motion sample + scan-match score (score_body.h) and the grouped
// out-of-place landmark update side by side.  The two are bound by different units — the scorer by the texture addresser
// (gathers out of L2), the update by HBM writes — and neither needs the other's output: both start from the resample
// indices and the previous poses (the update works out its particles' motion samples itself).  As two launches they run one
// after the other (a second stream with an event fork and join costs more than it wins: DESIGN.md section 11.5); here the
// workgroups of both kinds are dealt out interleaved — of every `score_octets + ekf_octets` consecutive octets of workgroups
// (an octet = one workgroup per XCD) the scoring ones are spread evenly — so the gathers run in the shadow of the row
// stores.  Same bits as the two launches (same device functions).
// A survivor-rows frame (no row stores) of the flagship shape goes to frame_particle_kernel below instead: one kind of workgroup.

#include "ekf_group_body.h"
#include "ekf_split_body.h"
#include "score_body.h"
#include "pf_common.h"

namespace slam {

namespace {

struct FrontArgs {
    ScoreGrid g;
    const float *bx, *by;
    int nbeams;
    float* score;
    int32_t* count;
    MotionIO mio;
    MotionParams mpar;
    EkfArgs a;
    int score_blocks;    // 256-thread slices of poses to score
    int score_octets;    // ceil(score_blocks / 8)
    int ekf_octets;      // update workgroups per XCD (the xcd_chunk of ekf_update_group_kernel)
    int score_span;      // the scoring octets lie among the first score_span octets of the grid
    float* obs_save;     // MEANS = false: [2][plane_stride], the observation table as this frame's update saw it
};

// the workgroup behind the grid of a survivor-rows frame's front launch: the observation table as this frame's update saw it, kept
// for the launch that writes the survivors' rows later (the caller's table may be rewritten as soon as the frame is issued)
__device__ __forceinline__ void obs_save_body(const FrontArgs& f, int threads)
{
    const int L = f.a.nlandmarks, Lp = f.a.plane_stride;
    const float nan = __uint_as_float(0x7fc00000u);
    for (int l = (int)threadIdx.x; l < Lp; l += threads) {
        f.obs_save[l] = l < L ? f.a.obs_zx[l] : nan;
        f.obs_save[Lp + l] = l < L ? f.a.obs_zy[l] : nan;
    }
}

// MEANS = false (split only): a survivor-rows frame — the updating workgroups write no mean row (ekf_split_body), and one workgroup
// behind the grid keeps a copy of the observation table for the launch that writes the survivors' rows later
constexpr int front_wpe(bool split, bool means) { return !split ? kEkfGroupWpe : means ? kEkfSplitWpe : kEkfSplitWpeNoStore; }

template <int NB, int G, int LPP, int DEPTH, bool SPLIT = false, bool PACKED = false, bool MEANS = true>
__global__ __launch_bounds__(kEkfWaves * 64) __attribute__((amdgpu_waves_per_eu(front_wpe(SPLIT, MEANS), front_wpe(SPLIT, MEANS))))
void frame_front_kernel(FrontArgs f)
{
    static_assert(kScoreBlock == kEkfWaves * 64, "both kinds of workgroup have 256 threads");
    extern __shared__ float4 s_pair[];
    __shared__ float s_acc[kEkfWaves][G][128];
    // a workgroup's motion samples, made once by one of its wavefronts: (x, y, sine, cosine) of the kScoreBlock / 4 poses of a
    // scoring workgroup with four lanes per pose, of the kEkfWaves * G particles of an updating one (1 KB)
    __shared__ float4 s_motion[kScoreBlock / 4];
    static_assert(kEkfWaves * G <= kScoreBlock / 4, "s_motion holds an updating workgroup's particles");
    if constexpr (!MEANS) {
        if (blockIdx.x == gridDim.x - 1) {
            obs_save_body(f, kEkfWaves * 64);
            return;
        }
    }
    const int o = (int)blockIdx.x >> 3, xcd = (int)blockIdx.x & 7;
    // the scoring octets are spread evenly over the first `span` octets of the grid: the whole grid (against the first part of it
    // only — 64k x 500, 4 / 2 particles per updating wavefront: 100 % 130.7 / 158.5 us, 75 % 134.0 / 156.3, 50 % 155.1 / 154.8,
    // 25 % 141.2 / 157.9)
    const int64_t span = f.score_span;
    const int before = o < span ? (int)((int64_t)o * f.score_octets / span) : f.score_octets;             // scoring octets among 0 .. o - 1
    const int upto = o + 1 < span ? (int)((int64_t)(o + 1) * f.score_octets / span) : f.score_octets;    // ... among 0 .. o
    if (upto > before) {   // a scoring octet (wave-uniform, workgroup-uniform)
        const int sb = before * 8 + xcd;
        if (sb >= f.score_blocks) return;
        score_poses_body<false, LPP, DEPTH, true, PACKED>(f.g, f.bx, f.by, f.nbeams, f.mio.x, f.mio.y, f.mio.th, nullptr, f.a.n,
                                                          f.score, f.count, f.mio, f.mpar, sb, s_pair, s_motion);
    } else if constexpr (SPLIT) {
        ekf_split_body<NB, G, kPosesMade, MEANS>(f.a, xcd * f.ekf_octets + (o - before), s_acc, f.mio, f.mpar, s_motion);
    } else {
        ekf_group_body<NB, G, true>(f.a, xcd * f.ekf_octets + (o - before), s_acc, f.mio, f.mpar);
    }
}

// ---- A particle's score, its landmark update and its weight in ONE workgroup (a survivor-rows frame of the split layout, 8 particles
// per wavefront, four lanes per pose): workgroup b owns particles [64 b, 64 b + 64), XCD-contiguous as the updating workgroups
// above.  With MEANS = false the launch stores no rows, so there is no HBM traffic left for the gathers to hide behind (the
// reason for the two kinds of workgroup above); and a score and a log-likelihood that come out of the same workgroup meet in LDS,
// which saves the weights' launch and the second motion sample of every particle.
//   stage: beams, decode table, the 64 motion samples by the last wavefront (score_stage), barrier;
//   S: the scorer on the 64 poses (score_poses_body, STAGED), every quad's score also into s_score;
//   U: each wavefront updates groups `wave` and `wave + 4` of the workgroup's eight groups of eight, one after the other, the
//      poses from the staged samples (ekf_split_group, kPosesStaged), every particle's log-likelihood also into s_ll;
//   barrier; W: thread t < 64 makes particle 64 b + t's log-weight (log_weight_of) and the first wavefront the block's maximum
//      (the per-element rule of logweight_kernel, then fmaxf across the lanes: the maximum of a set, however it is blocked).
// The workgroups whose blockIdx.x has bit 8 set run U before S, so that neighbours on a compute unit gather while the others compute:
// an XCD's workgroups (blockIdx.x >> 3 = 0, 1, ..) are dealt to its 32 compute units in turn, so with all of the bench shape's 1 024
// workgroups resident at once, 4 per unit, the four of a unit are 32 apart there and two of them run each order.  For other
// populations (fewer than 4 per unit, or a second round) neighbours need not alternate: the results are the same bits either way,
// the measured gain belongs to 65 536 particles.  (The same order in every workgroup was measured and dropped: figures below.)
// The same device functions on the same inputs as the kernels above plus logweight_cov_kernel: the same bits.
// Measured (profiles/r09_front_combined.md; ms per frame at 64k x 500, medians of four interleaved runs, the separate
// launches 0.0752): S before U everywhere 0.0761 at 4 waves per SIMD (98 VGPRs), 0.0762 at 5 (95), 0.0785 at 6 (80);
// alternating at 4 waves (99 VGPRs) 0.0728.  1 024 workgroups are 4 per compute unit, one wavefront per SIMD each.
constexpr int kFrontParticleWpe = 4;
constexpr int kFrontParticleG = 8;

template <bool PACKED>
__global__ __launch_bounds__(kScoreBlock) __attribute__((amdgpu_waves_per_eu(kFrontParticleWpe, kFrontParticleWpe)))
void frame_particle_kernel(FrontArgs f, FrontWeights w)
{
    constexpr int G = kFrontParticleG, kOwn = kScoreBlock / 4;   // particles of a workgroup
    static_assert(kOwn == 2 * kEkfWaves * G, "every wavefront takes two groups");
    extern __shared__ float4 s_pair[];
    __shared__ float s_acc[kEkfWaves][G][128];
    __shared__ float4 s_motion[kOwn];
    __shared__ float s_score[kOwn], s_ll[kOwn];
    if (blockIdx.x == gridDim.x - 1) {
        obs_save_body(f, kScoreBlock);
        return;
    }
    const int n = f.a.n;
    const int b = xcd_block(f.a.xcd_chunk), first = b * kOwn;
    if (first >= n) return;   // (a surplus workgroup of the padded grid)
    score_stage<4, kQuadDepth, true, PACKED>(f.g, f.bx, f.by, f.nbeams, f.mio.x, f.mio.y, f.mio.th, n, f.mio, f.mpar, b, s_pair, s_motion);
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int flip = ((int)blockIdx.x >> 8) & 1;
#pragma nounroll
    for (int step = 0; step < 2; ++step) {
        if ((step ^ flip) == 0) {
            score_poses_body<false, 4, kQuadDepth, true, PACKED, true>(f.g, f.bx, f.by, f.nbeams, f.mio.x, f.mio.y, f.mio.th, nullptr, n,
                                                                       f.score, f.count, f.mio, f.mpar, b, s_pair, s_motion, s_score);
        } else {
#pragma nounroll
            for (int r = 0; r < 2; ++r)
                ekf_split_group<kEkfSplitNb, G, kPosesStaged, false>(f.a, first, wave + kEkfWaves * r, wave, s_acc, f.mio, f.mpar, s_motion,
                                                                     s_ll);
        }
    }
    __syncthreads();
    if (threadIdx.x >= 64) return;
    const int t = (int)threadIdx.x, i = first + t;
    const bool add_carry = w.carry && *w.prev_resampled == 0;
    float m = -INFINITY;
    if (i < n) {
        const float lw = log_weight_of(s_ll[t], s_score[t] * w.gain, w.carry, add_carry, i);
        w.logw[i] = lw;
        m = lw > m ? lw : m;
    }
    m = wave_max(m);
    if (t == 0) w.block_max[b] = m;
}

int update_blocks(int n, int group_size) { return (n + kEkfWaves * group_size - 1) / (kEkfWaves * group_size); }
}  // namespace

bool frame_front_fits(int n, int nlandmarks, int group_size)
{
    if (n < kWaveMaxPoses || nlandmarks <= 128 || (group_size != 2 && group_size != 4 && group_size != 8)) return false;
    return update_blocks(n, group_size) >= 64;
}

// The front of a single-GPU frame in one launch (frame_front_kernel).  *launched = false when the shapes do not fit it (few
// particles: the one-wavefront-per-pose scorer; short rows; too few update workgroups for the XCD-contiguous numbering): the
// caller then issues the two launches.
hipError_t launch_frame_front(hipStream_t stream, const ScoreGrid& g, const float* bx, const float* by, int nbeams,
                              const MotionIO& io, int64_t first_id, const float dp[3], const float sigma[3], uint64_t seed,
                              uint32_t frame, float* score, int32_t* count, const EkfArgs& a_in, int group_size,
                              const EventPair* ev, bool* launched, int* lanes_per_pose, float* obs_save, const FrontWeights* weights)
{
    *launched = false;
    if (weights) *weights->made = false;
    const int n = a_in.n;
    if (!a_in.cov && group_size == 8) group_size = 4;   // rows: 2 or 4 particles per updating wavefront
    if (a_in.map_in == a_in.map_out || !frame_front_fits(n, a_in.nlandmarks, group_size)) return hipSuccess;
    if (obs_save && !a_in.cov) return hipErrorInvalidValue;   // survivor rows are a mode of the split layout
    const int G = group_size;
    const bool quad = n < kQuadMaxPoses;
    FrontArgs f;
    f.g = g;
    f.bx = bx;
    f.by = by;
    f.nbeams = nbeams;
    f.score = score;
    f.count = count;
    f.mio = io;
    f.mpar = make_motion_params(first_id, dp, sigma, seed, frame);
    f.a = a_in;
    f.ekf_octets = (update_blocks(n, G) + 7) / 8;
    f.a.xcd_chunk = f.ekf_octets;
    f.score_blocks = (int)(((quad ? 4L : 1L) * n + kScoreBlock - 1) / kScoreBlock);
    f.score_octets = (f.score_blocks + 7) / 8;
    f.score_span = f.score_octets + f.ekf_octets;
    f.obs_save = obs_save;
    const int grid = 8 * f.score_span + (obs_save ? 1 : 0);
    const size_t lds = sizeof(float2) * (size_t)(nbeams + (quad ? 4 * kQuadDepth : kLaneDepth)) + (g.packed ? 1024 : 0);
    if (ev) (void)hipEventRecord(ev->start, stream);
    // one workgroup per 64 particles, weights included (frame_particle_kernel), where the frame allows it
    if (weights && weights->logw && weights->block_max && obs_save && f.a.cov && G == kFrontParticleG && quad && f.a.group_filter == 0 &&
        (n + 63) / 64 <= kMaxWeightBlocks) {
        f.a.xcd_chunk = ((n + 63) / 64 + 7) / 8;
        const int pgrid = 8 * f.a.xcd_chunk + 1;
        if (f.g.packed) frame_particle_kernel<true><<<pgrid, kScoreBlock, lds, stream>>>(f, *weights);
        else frame_particle_kernel<false><<<pgrid, kScoreBlock, lds, stream>>>(f, *weights);
        if (ev) (void)hipEventRecord(ev->stop, stream);
        *launched = true;
        *weights->made = true;
        if (lanes_per_pose) *lanes_per_pose = 4;
        return hipGetLastError();
    }
    // the instantiation: particles per updating wavefront (8: split only) x scorer's lane mapping x map layout x grid copy read
    // ... x mean rows written or not (split only)
#define SLAM_FRONT(G_, SP_, PK_, MN_)                                                                                             \
    do {                                                                                                                          \
        constexpr int NB_ = (SP_) ? kEkfSplitNb : kEkfGroupNb;                                                                    \
        if (quad) frame_front_kernel<NB_, G_, 4, kQuadDepth, SP_, PK_, MN_><<<grid, kEkfWaves * 64, lds, stream>>>(f);            \
        else frame_front_kernel<NB_, G_, 1, kLaneDepth, SP_, PK_, MN_><<<grid, kEkfWaves * 64, lds, stream>>>(f);                 \
    } while (0)
#define SLAM_FRONT_PK(G_, SP_, MN_) do { if (f.g.packed) SLAM_FRONT(G_, SP_, true, MN_); else SLAM_FRONT(G_, SP_, false, MN_); } while (0)
#define SLAM_FRONT_SPLIT(G_) do { if (obs_save) SLAM_FRONT_PK(G_, true, false); else SLAM_FRONT_PK(G_, true, true); } while (0)
    if (G == 2) { if (f.a.cov) SLAM_FRONT_SPLIT(2); else SLAM_FRONT_PK(2, false, true); }
    else if (G == 8 && f.a.cov) SLAM_FRONT_SPLIT(8);
    else if (f.a.cov) SLAM_FRONT_SPLIT(4);
    else SLAM_FRONT_PK(4, false, true);
#undef SLAM_FRONT_SPLIT
#undef SLAM_FRONT_PK
#undef SLAM_FRONT
    if (ev) (void)hipEventRecord(ev->stop, stream);
    *launched = true;
    if (lanes_per_pose) *lanes_per_pose = quad ? 4 : 1;
    return hipGetLastError();
}

}  // namespace slam
