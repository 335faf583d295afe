// localise_kernels.hip — localisation in a known landmark map (no counterpart in the reference; specification:
// tests/_localise_spec.py).  Every particle associates the frame's detections with ONE map all particles
// share and takes the matched pairs' log-likelihood; the map is never changed.  With one map and meas_var * I noise nothing that
// involves a covariance depends on the particle, so it is worked out once per map, not once per (particle, landmark, frame):
//
// known_map_prepare_kernel: M [5][stride] -> the prepared map [6][stride] = mx, my, i00, i01, i11, hl with S^-1 = (P + q I)^-1 and
// hl = 0.5 log det S: the operations of ekf_det_terms / ekf_shared_from (ekf_rcp, det_logf), the bits the specification computes
// per particle.  A slot that holds no landmark (P_xx < 0) and the padding behind L get a NaN mean: they take no part (match_body.h).
//
// localise_kernel: the matching of match_body.h (a wavefront per particle at a time; steps a, c, d and the table row are its
// functions) on that one map, without rows; det_sincosf once per particle.  What is the stage's own:
//   e. lane k holds detection k's winner: its term ((0 - 0.5 m) - hl) - log 2 pi from the m in the key and one read of hl, added
//      to accumulator l mod 128 in ascending l — batch by batch, batches without a winner skipped: what they would add is +0 to an
//      accumulator that is never -0 — then accumulators j and j + 64 and the xor butterfly: orc_ekf_update's order.
// The workgroups are persistent (a grid that fills the machine once, each wavefront takes particles a grid apart), so the prepared
// map is staged in LDS once per workgroup where it fits (24 B per landmark, padded to whole batches: nothing is predicated) and
// read from memory, L2-resident, where it does not.  No row is read and none is written: a frame without a table pointer reads
// 12 B and writes 16 B per particle.
//
// Under a covariance PER DETECTION (specification: tests/_localise_detcov_spec.py) S = P + R_w(theta_i, k) depends on the particle
// and the detection, nothing can be prepared, and localise_detcov_kernel is the same body on the RAW map [5][stride]: the noise is
// AssocNoiseDet (assoc_noise.h: lane k forms R_w(theta_i, k) once, beside its world point; the loop over k reads point and noise as
// wave-uniform values and forms (P + R_w)^-1 per (landmark, detection) pair — the two landmarks of a lane are the two independent
// reciprocal chains in flight; ekf_rcp's wave-uniform range test is a branch, which keeps the loop from being unrolled across
// detections), a slot without a landmark gets its NaN mean where the map is read
// (staged: once per workgroup, 20 B per landmark), and lane k rebuilds its winner's det S from one read of the landmark's three
// covariance planes and its own R_w for hl = 0.5 log det S.  Everything else — minima, accumulation order, stats, table — is shared.
//
// THE MISS FORM of both (localise_miss_kernel, localise_detcov_miss_kernel; specification: tests/_localise_miss_spec.py) also counts,
// in the same launch, what the map says the pose should have seen and no detection matched: the seen landmarks within view_range
// that are no detection's winner — outside the arc, spared by line of sight, or missed — under the evidence stage's predicate
// (evidence_visibility of evidence_common.h, the one copy).  The winners are at most K distinct landmarks, so nothing is kept per
// landmark: the matching pass counts the classes of every landmark by ballot while it holds the means, and lane k takes its
// winner out of its class again.  MISS is compile time — the four kernels without it are the code they were — and so is DIR,
// "some direction test is on": without it (range only) none of the direction code is compiled in; with it the arc and line of
// sight are wave-uniform run-time switches (profiles/localise_miss.md).  It adds the sight table (at most 4 KB,
// staged in front of the workgroup's barrier) to the LDS and nothing else: loc_lds below lays out and sizes every form.

#include "assoc_noise.h"
#include "evidence_common.h"
#include "match_body.h"

namespace slam {

namespace {

constexpr unsigned kLocStagedMax = 2048;   // landmarks (whole batches) up to which the prepared map is staged: 48 KB

// LDS of one workgroup, in multiples of 16 bytes: [staged: map `planes` x Lr floats] | [MISS with line of sight: the sight table,
// sight_bins floats] | per wavefront: best[64] u64 | acc[128] float | [table wanted: row[L rounded up to 16] u8].  The misses keep
// nothing per landmark (see localise_particle), so the miss form adds the sight table and nothing else
struct LocLds {
    unsigned batches, Lr, rowb, map_bytes, sight_bytes, per_wave;
    __host__ __device__ constexpr unsigned front() const { return map_bytes + sight_bytes; }                       // what the wavefronts share
    __host__ __device__ constexpr unsigned total() const { return front() + (unsigned)kEkfWaves * per_wave; }      // the launch's request
};
__host__ __device__ constexpr inline LocLds loc_lds(unsigned L, bool staged, bool table, unsigned planes, unsigned sight_bins = 0u)
{
    LocLds s{};
    s.batches = (L + 127u) / 128u;
    s.Lr = s.batches * 128u;
    s.rowb = table ? (L + 15u) & ~15u : 0u;
    s.map_bytes = staged ? planes * 4u * s.Lr : 0u;
    s.sight_bytes = sight_bins * 4u;
    s.per_wave = 64u * 8u + 128u * 4u + s.rowb;
    return s;
}
// the two worst cases — the largest staged prepared map and the largest map read from memory, each with a table row and the largest
// sight table — fit a workgroup's 64 KB: no launch the launchers below can size asks for more
static_assert(loc_lds(kLocStagedMax, true, true, 6u, (unsigned)kSightMaxBins).total() <= 65536u, "staged form: LDS");
static_assert(loc_lds((unsigned)SLAM_MAX_OBS, false, true, 6u, (unsigned)kSightMaxBins).total() <= 65536u, "from-memory form: LDS");

__global__ __launch_bounds__(256) void known_map_prepare_kernel(KnownMapArgs a)
{
    const int l = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (l >= a.plane_stride) return;
    const size_t ps = (size_t)a.plane_stride;
    const bool in = l < a.nlandmarks;
    const float nan = __uint_as_float(0x7fc00000u);
    // (padding: the identity, whose terms are finite — the values are never read as a landmark's)
    const float mx = in ? a.map[l] : 0.0f, my = in ? a.map[ps + l] : 0.0f;
    const float pxx = in ? a.map[2 * ps + l] : 1.0f, pxy = in ? a.map[3 * ps + l] : 0.0f, pyy = in ? a.map[4 * ps + l] : 1.0f;
    float idet, hl;
    ekf_det_terms<float>(pxx, pxy, pyy, a.meas_var, idet, hl);
    const EkfShared<float> h = ekf_shared_from<float, false>(pxx, pxy, pyy, a.meas_var, idet, hl);
    const bool seen = in && !(pxx < 0.0f);   // the update's own first-sighting test
    a.prep[l] = seen ? mx : nan;
    a.prep[ps + l] = my;
    a.prep[2 * ps + l] = h.i00;
    a.prep[3 * ps + l] = h.i01;
    a.prep[4 * ps + l] = h.i11;
    a.prep[5 * ps + l] = h.hl;
}

// the map as a wavefront reads it: the two landmarks of a lane in batch b (planes 0 .. 4), and one plane of one landmark.
// RAW: the map as it was given (mx, my, P_xx, P_xy, P_yy), else the prepared one (mx, my, i00, i01, i11, hl)
struct LocMapLds {
    const float* s;   // [planes][Lr], NaN means from L on and (RAW) where the slot holds no landmark
    unsigned Lr;
    __device__ __forceinline__ void pair(unsigned b, unsigned lane, v2f (&m)[5]) const
    {
        const unsigned l = b * 128u + lane;
#pragma unroll
        for (int p = 0; p < 5; ++p) m[p] = (v2f){s[(unsigned)p * Lr + l], s[(unsigned)p * Lr + l + 64u]};
    }
    __device__ __forceinline__ float plane(unsigned p, unsigned l) const { return s[p * Lr + l]; }
};
template <bool RAW> struct LocMapMem {
    const float* g;   // [planes][ps]
    unsigned ps, L;
    __device__ __forceinline__ void pair(unsigned b, unsigned lane, v2f (&m)[5]) const
    {
        const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const unsigned l = b * 128u + 64u * t + lane;
            const bool in = l < L;
            const unsigned c = in ? l : 0u;   // clamped index + select instead of a predicated load
#pragma unroll
            for (int p = 0; p < 5; ++p) m[p][t] = g[(size_t)p * ps + c];
            m[0][t] = in && !(RAW && m[2][t] < 0.0f) ? m[0][t] : nan;   // (RAW: the update's own first-sighting test)
        }
    }
    __device__ __forceinline__ float plane(unsigned p, unsigned l) const { return g[(size_t)p * ps + l]; }
};

// The noise of the stage, a policy in the shape of assoc_noise.h's: LocNoisePrepared — meas_var * I, S^-1 and hl are planes 2 .. 5
// of the prepared map — or AssocNoiseDet on the raw map
struct LocNoisePrepared {
    static constexpr bool kPerDetection = false;
    __device__ __forceinline__ LocNoisePrepared(const DetCovArgs&, float, float) {}
    __device__ __forceinline__ EkfShared<v2f> inverse(v2f m2, v2f m3, v2f m4) const
    {
        EkfShared<v2f> h;   // (only S^-1 is filled in)
        h.i00 = m2;
        h.i01 = m3;
        h.i11 = m4;
        return h;
    }
};
// 0.5 log det S of lane k's winner wl
template <class MAP> __device__ __forceinline__ float loc_half_logdet(const LocNoisePrepared&, const MAP& map, unsigned wl) { return map.plane(5u, wl); }
template <class MAP> __device__ __forceinline__ float loc_half_logdet(const AssocNoiseDet& r, const MAP& map, unsigned wl)
{
    const float a = map.plane(2u, wl) + r.rxx, b = map.plane(3u, wl) + r.rxy, cc = map.plane(4u, wl) + r.ryy;   // ekf_aniso_update_one's det
    const float det = a * cc - b * b;
    return 0.5f * ekf_log(det);
}

// MISS: the landmarks the map says the pose should have seen and no detection matched (specification:
// tests/_localise_miss_spec.py) — the evidence stage's predicate (evidence_visibility), counted per class.  A landmark is hit
// exactly where it is some detection's winner, and the winners are at most K distinct landmarks, so nothing is kept per landmark:
// the matching pass, which holds every mean in registers, counts the classes of ALL landmarks in range, and lane k then takes its
// winner out of the class the same function puts it in (the same inputs, the same bits).  fov and sight are wave-uniform run-time
// switches of the one MISS form
template <class NOISE, bool MISS, bool DIR, class MAP>
__device__ __forceinline__ void localise_particle(const LocaliseArgs& a, const DetCovArgs& q, const LocMissArgs& v, const float* s_tab, const MAP& map,
                                                  int i, unsigned lane, const LocLds& lds, u64* s_best, float* s_acc, unsigned char* s_row)
{
    const unsigned K = (unsigned)a.ndet;
    wave_lds_sync();   // (the particle before this one has read what is written here)
    match_reset(s_best, s_row, lds.rowb, lane);
    s_acc[lane] = 0.0f;
    s_acc[lane + 64u] = 0.0f;

    float st, ct;
    det_sincosf(a.th[i], st, ct);
    float wxk, wyk;
    match_world_point(a.det_zx, a.det_zy, K, lane, st, ct, a.x[i], a.y[i], wxk, wyk);
    const NOISE noise(q, st, ct);   // (per detection: lane k's R_w(theta_i, k))
    [[maybe_unused]] EvidenceView view{};
    [[maybe_unused]] const bool fov = MISS && DIR && v.fov != 0, sight = MISS && DIR && v.bins != 0;
    [[maybe_unused]] int nmissed = 0, nspared = 0, noutside = 0;
    if constexpr (MISS)
        view = EvidenceView{ a.x[i], a.y[i], st, ct, v.range2, v.lo, v.hi, v.lo > v.hi, s_tab, (float)(v.bins >> 2), (unsigned)v.bins - 1u, v.margin };

    const float inf = __uint_as_float(0x7f800000u);
    for (unsigned b = 0; b < lds.batches; ++b) {
        v2f m[5];
        map.pair(b, lane, m);
        if constexpr (MISS) {   // every landmark as if no detection had matched it (a NaN mean is not in range)
            const float mx[2] = { m[0][0], m[0][1] }, my[2] = { m[1][0], m[1][1] };
            const bool open[2] = { true, true };
            bool due[2], in_view[2], hidden[2];
            evidence_visibility<2>(view, fov, sight, mx, my, open, due, in_view, hidden);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                nmissed += __popcll(__ballot(due[t] && in_view[t] && !hidden[t]));
                nspared += __popcll(__ballot(hidden[t]));
                noutside += __popcll(__ballot(due[t] && !in_view[t]));
            }
        }
        // b. S^-1: the prepared one — or (P + R_w(theta_i, k))^-1 per pair inside the loop
        EkfShared<v2f> h;
        if constexpr (!NOISE::kPerDetection) h = noise.inverse(m[2], m[3], m[4]);
        v2f best = bc2(inf);
        unsigned bk[2] = { 0u, 0u };
        for (unsigned k = 0; k < K; ++k) {
            v2f wx, wy;
            match_point(wxk, wyk, k, wx, wy);
            if constexpr (NOISE::kPerDetection) h = noise.inverse(m[2], m[3], m[4], k);
            match_pair(wx, wy, k, m[0], m[1], h, best, bk);
        }
        match_post(s_best, best, bk, a.gate, b * 128u + lane);
    }
    wave_lds_sync();

    // e. lane k: detection k's winner and its term (m = +0 where it was -0: the two subtractions behind it erase that sign)
    const MatchWinner won = match_winner(s_best, lane, K);
    const bool matched = won.matched;
    const unsigned wl = won.l;
    float term = 0.0f;
    if (matched) {
        term = (-(0.5f * __uint_as_float(won.mbits)) - loc_half_logdet(noise, map, wl)) - 1.8378770664f;
        if (lds.rowb) s_row[wl] = (unsigned char)lane;
    }
    if constexpr (MISS) {   // ... and the winners, which are hit, out of their classes again.  (A lane without a winner reads
        // landmark 0 — match_winner's l is 0 where nothing matched, in bounds for every L >= 1 — and is closed by open = matched)
        const float mx[1] = { map.plane(0u, wl) }, my[1] = { map.plane(1u, wl) };
        const bool open[1] = { matched };
        bool due[1], in_view[1], hidden[1];
        evidence_visibility<1>(view, fov, sight, mx, my, open, due, in_view, hidden);
        nmissed -= __popcll(__ballot(due[0] && in_view[0] && !hidden[0]));
        nspared -= __popcll(__ballot(hidden[0]));
        noutside -= __popcll(__ballot(due[0] && !in_view[0]));
    }
    const u64 mm = __ballot(matched);
    const int nmatched = __popcll(mm);
    if (mm != 0)
        for (unsigned b = 0; b < lds.batches; ++b) {
            const bool mine = matched && (wl >> 7) == b;   // at most one winner per accumulator and batch
            if (__ballot(mine) == 0) continue;
            if (mine) s_acc[wl & 127u] = s_acc[wl & 127u] + term;
            wave_lds_sync();
        }
    wave_lds_sync();
    const float total = wave_xor_tree_sum(s_acc[lane] + s_acc[lane + 64u]);
    if (lane == 0) {
        a.loglik[i] = total;
        int32_t* st3 = a.stats + 3 * (size_t)i;
        st3[0] = nmatched;
        st3[1] = 0;
        st3[2] = (int)K - nmatched;
        if constexpr (MISS) {
            v.missed[i] = nmissed;
            if (v.spared) v.spared[i] = nspared;
            if (v.outside) v.outside[i] = noutside;
        }
    }
    if (lds.rowb) match_row_write(s_row, lds.rowb, a.assoc, i, (unsigned)a.assoc_stride, lane);
}

// RAW: a.map is the map as it was given and NOISE reads q; else the prepared map (q is not read)
// MISS: v is read, and the sight table (v.bins floats; 0: no line of sight) is staged in front of the workgroup's barrier — the one
// the staged map has, or the one barrier the form that reads the map from memory gains
template <bool STAGED, bool RAW, bool MISS, bool DIR, class NOISE>
__device__ __forceinline__ void localise_body(const LocaliseArgs& a, const DetCovArgs& q, const LocMissArgs& v)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr unsigned kPlanes = RAW ? 5u : 6u;
    const unsigned lane = threadIdx.x & 63u;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned L = (unsigned)a.nlandmarks;
    const LocLds lds = loc_lds(L, STAGED, a.assoc != nullptr, kPlanes, MISS ? (unsigned)v.bins : 0u);
    unsigned char* mine = smem + (MISS ? lds.front() : lds.map_bytes) + (unsigned)wave * lds.per_wave;
    u64* s_best = reinterpret_cast<u64*>(mine);
    float* s_acc = reinterpret_cast<float*>(s_best + 64);
    unsigned char* s_row = reinterpret_cast<unsigned char*>(s_acc + 128);
    const int first = (int)blockIdx.x * kEkfWaves + wave, step = (int)gridDim.x * kEkfWaves;
    float* s_tab = reinterpret_cast<float*>(smem + lds.map_bytes);
    if constexpr (MISS && DIR)
        for (int j = (int)threadIdx.x; j < v.bins; j += kEkfWaves * 64) s_tab[j] = v.table[j];
    if constexpr (STAGED) {
        float* s_map = reinterpret_cast<float*>(smem);
        const float nan = __uint_as_float(0x7fc00000u);
        const size_t ps = (size_t)a.plane_stride;
        for (unsigned l = threadIdx.x; l < lds.Lr; l += kEkfWaves * 64u) {
            // (RAW padding: P = I, whose terms are finite — the values are never read as a landmark's)
            const bool seen = l < L && !(RAW && a.map[2 * ps + l] < 0.0f);
#pragma unroll
            for (unsigned p = 0; p < kPlanes; ++p) {
                const float pad = RAW && (p == 2u || p == 4u) ? 1.0f : 0.0f;
                s_map[p * lds.Lr + l] = p == 0u ? (seen ? a.map[l] : nan) : (l < L ? a.map[p * ps + l] : pad);
            }
        }
        __syncthreads();   // (the only workgroup barrier: from here on a wavefront is on its own)
        const LocMapLds map{ s_map, lds.Lr };
        for (int i = first; i < a.n; i += step) localise_particle<NOISE, MISS, DIR>(a, q, v, s_tab, map, i, lane, lds, s_best, s_acc, s_row);
    } else {
        if constexpr (MISS && DIR) __syncthreads();   // (the sight table)
        const LocMapMem<RAW> map{ a.map, (unsigned)a.plane_stride, L };
        for (int i = first; i < a.n; i += step) localise_particle<NOISE, MISS, DIR>(a, q, v, s_tab, map, i, lane, lds, s_best, s_acc, s_row);
    }
}

template <bool STAGED> __global__ __launch_bounds__(kEkfWaves * 64) void localise_kernel(LocaliseArgs a)
{
    localise_body<STAGED, false, false, false, LocNoisePrepared>(a, DetCovArgs{}, LocMissArgs{});
}
// DIR: the arc and line of sight are run-time switches of the form; else neither is compiled in (range only)
template <bool STAGED, bool DIR> __global__ __launch_bounds__(kEkfWaves * 64) void localise_miss_kernel(LocaliseArgs a, LocMissArgs v)
{
    localise_body<STAGED, false, true, DIR, LocNoisePrepared>(a, DetCovArgs{}, v);
}

// ... on the raw map under S = P + R_w(theta_i, k), Q_k per detection
template <bool STAGED> __global__ __launch_bounds__(kEkfWaves * 64) void localise_detcov_kernel(LocaliseArgs a, DetCovArgs q)
{
    localise_body<STAGED, true, false, false, AssocNoiseDet>(a, q, LocMissArgs{});
}
template <bool STAGED, bool DIR> __global__ __launch_bounds__(kEkfWaves * 64) void localise_detcov_miss_kernel(LocaliseArgs a, DetCovArgs q, LocMissArgs v)
{
    localise_body<STAGED, true, true, DIR, AssocNoiseDet>(a, q, v);
}

// the launch of one of the twelve kernels: a grid that fills the machine once — as many workgroups as are resident together, or as
// the particles need
template <class KERNEL, class... MORE>
hipError_t loc_launch(KERNEL kernel, hipStream_t stream, const LocaliseArgs& a, size_t lds, const EventPair* ev, const MORE&... more)
{
    const int need = (a.n + kEkfWaves - 1) / kEkfWaves;
    int dev = 0, cus = 0, per_cu = 0;
    hipError_t err = hipGetDevice(&dev);
    if (err == hipSuccess) err = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (err == hipSuccess) err = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, kEkfWaves * 64, lds);
    if (err != hipSuccess) return err;
    const int64_t resident = (int64_t)cus * per_cu;
    const int blocks = resident > 0 && resident < need ? (int)resident : need;
    if (ev) (void)hipEventRecord(ev->start, stream);
    kernel<<<blocks, kEkfWaves * 64, lds, stream>>>(a, more...);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

}  // namespace

bool localise_args_ok(const LocaliseArgs& a)
{
    return !(a.nlandmarks < 1 || a.nlandmarks > SLAM_MAX_OBS || a.plane_stride < a.nlandmarks || a.ndet < 0 ||
             a.ndet > SLAM_MAX_DETECTIONS || (a.assoc && a.assoc_stride < a.nlandmarks) || !a.map || !a.stats || !a.loglik);
}

hipError_t launch_known_map_prepare(hipStream_t stream, const KnownMapArgs& a, const EventPair* ev)
{
    if (a.nlandmarks < 1 || a.nlandmarks > SLAM_MAX_OBS || a.plane_stride < a.nlandmarks || !a.map || !a.prep) return hipErrorInvalidValue;
    if (ev) (void)hipEventRecord(ev->start, stream);
    known_map_prepare_kernel<<<(a.plane_stride + 255) / 256, 256, 0, stream>>>(a);
    if (ev) (void)hipEventRecord(ev->stop, stream);
    return hipGetLastError();
}

hipError_t launch_localise(hipStream_t stream, const LocaliseArgs& a, const DetCovArgs* q, const LocMissArgs* v, const EventPair* ev)
{
    if (a.n <= 0) return hipSuccess;
    if (!localise_args_ok(a) || (q && (q->ndet != a.ndet || (q->ndet > 0 && (!q->qxx || !q->qxy || !q->qyy))))) return hipErrorInvalidValue;
    // the misses: what the predicate and the staging of the sight table are sized by (v->bins floats of LDS and of v->table)
    if (v && (!v->missed || !(v->range2 > 0.0f) || (v->fov && !fov_bounds_ok(v->lo, v->hi)) ||
              (v->table ? !sight_bins_ok(v->bins) || !(v->margin > 0.0f) : v->bins != 0)))
        return hipErrorInvalidValue;
    const bool staged = (unsigned)(a.nlandmarks + 127) / 128u * 128u <= kLocStagedMax;   // (either map: 48 KB prepared, 40 KB raw)
    const LocLds s = loc_lds((unsigned)a.nlandmarks, staged, a.assoc != nullptr, q ? 5u : 6u, v ? (unsigned)v->bins : 0u);
    const size_t lds = s.total();   // at most 60 KB staged and 36 KB from memory; with the largest sight table 64 KB and 40 KB
    if (v) {
        const bool dir = v->fov || v->bins;   // the landmark's direction in the sensor frame is needed
        if (q) {
            const auto kernel = staged ? (dir ? localise_detcov_miss_kernel<true, true> : localise_detcov_miss_kernel<true, false>)
                                       : (dir ? localise_detcov_miss_kernel<false, true> : localise_detcov_miss_kernel<false, false>);
            return loc_launch(kernel, stream, a, lds, ev, *q, *v);
        }
        const auto kernel = staged ? (dir ? localise_miss_kernel<true, true> : localise_miss_kernel<true, false>)
                                   : (dir ? localise_miss_kernel<false, true> : localise_miss_kernel<false, false>);
        return loc_launch(kernel, stream, a, lds, ev, *v);
    }
    if (q) return staged ? loc_launch(localise_detcov_kernel<true>, stream, a, lds, ev, *q) : loc_launch(localise_detcov_kernel<false>, stream, a, lds, ev, *q);
    return staged ? loc_launch(localise_kernel<true>, stream, a, lds, ev) : loc_launch(localise_kernel<false>, stream, a, lds, ev);
}

}  // namespace slam
