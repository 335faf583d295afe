// match_body.h — the matching of a frame's detections to the landmarks of ONE particle, as the associating kernels share it
// (associate_body of assoc_kernels.hip: the particle's own row, unseen slots, creation; localise_particle of
// localise_kernels.hip: one map for every particle, the matched pairs' log-likelihood).  ONE WAVEFRONT OWNS ONE PARTICLE, lanes
// own landmarks l and l + 64 of each batch of 128 and walk the K detections in a wave-uniform loop.  The steps, in the letters of
// DESIGN.md section 7 (the noise, step b, is a policy of assoc_noise.h; the source of the map and what becomes of the winners
// belong to the kernels):
//   a. match_world_point: lane k holds detection k in the world frame;
//   c. match_point, match_pair: every landmark keeps its cheapest detection (strict <, k ascending: the lowest k on ties, NaN never wins);
//   d. match_post: the candidates (0 <= m <= gate) post (bits(m) << 32 | l) to an LDS 64-bit minimum per detection — m >= 0, so
//      the order of the bits is the order of the values, -0 is made +0 first, and l in the low word breaks ties towards the lowest
//      landmark: the result does not depend on the order in which lanes or batches arrive;
//      match_winner: lane k reads detection k's winner back;
//   f. match_row_write: the particle's table row, assembled in LDS (match_reset: 255 everywhere, the winners' lanes on top), goes
//      out as whole dwords where every row starts on one.
// A LANDMARK THAT TAKES NO PART — a slot that holds none, the padding behind L — is given a NaN mean by whoever reads the map:
// every Mahalanobis term of its is NaN, NaN passes no comparison of step c, its best stays +inf, and +inf passes no <= gate of
// step d under a finite gate (the engine's entry points refuse any other).  No step tests "seen" again.
#pragma once

#include "ekf_wave.h"

namespace slam {

typedef unsigned long long u64;

// what one lane wrote to LDS, every lane of the SAME wavefront may read afterwards
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the minima and the first rowb bytes of the table row (rowb: a multiple of 16, 0: no table) before a particle's matching
__device__ __forceinline__ void match_reset(u64* s_best, unsigned char* s_row, unsigned rowb, unsigned lane)
{
    unsigned* s_row32 = reinterpret_cast<unsigned*>(s_row);
    s_best[lane] = ~0ull;
    for (unsigned d = lane; d < rowb / 4u; d += 64u) s_row32[d] = 0xffffffffu;
}

// a. lane k: detection k in the world frame (the observed point of ekf_particle / ekf_first_sighting)
__device__ __forceinline__ void match_world_point(const float* det_zx, const float* det_zy, unsigned K, unsigned lane, float st, float ct,
                                                  float px, float py, float& wxk, float& wyk)
{
    const float zxk = lane < K ? det_zx[lane] : 0.0f, zyk = lane < K ? det_zy[lane] : 0.0f;
    ekf_first_sighting<float>(zxk, zyk, st, ct, px, py, wxk, wyk);
}

// ... and detection k (wave-uniform) as every lane sees it.  A kernel whose S^-1 is per detection reads the point first: the
// readlanes then stand in front of the reciprocal chain, not behind it
__device__ __forceinline__ void match_point(float wxk, float wyk, unsigned k, v2f& wx, v2f& wy)
{
    wx = bc2(lane_value(wxk, (int)k));
    wy = bc2(lane_value(wyk, (int)k));
}

// c, for one k: the Mahalanobis term of a lane's two landmarks (means mx, my; h: S^-1 in i00 / i01 / i11) against detection k's
// point — the operations of ekf_particle, the same bits — folded into the landmarks' best / bk
__device__ __forceinline__ v2f match_pair(v2f wx, v2f wy, unsigned k, v2f mx, v2f my, const EkfShared<v2f>& h, v2f& best, unsigned (&bk)[2])
{
    const v2f dx = wx - mx, dy = wy - my;
    const v2f t0 = h.i00 * dx + h.i01 * dy, t1 = h.i01 * dx + h.i11 * dy;
    const v2f maha = dx * t0 + dy * t1;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const bool take = maha[t] < best[t];
        best[t] = take ? maha[t] : best[t];
        bk[t] = take ? k : bk[t];
    }
    return maha;
}

// d. the candidates among landmarks l0 and l0 + 64 post to their detection's minimum
__device__ __forceinline__ void match_post(u64* s_best, v2f best, const unsigned (&bk)[2], float gate, unsigned l0)
{
#pragma unroll
    for (int t = 0; t < 2; ++t)
        if (best[t] >= 0.0f && best[t] <= gate) {
            const unsigned bits = best[t] == 0.0f ? 0u : __float_as_uint(best[t]);   // -0 -> +0
            atomicMin(&s_best[bk[t]], ((u64)bits << 32) | (l0 + 64u * (unsigned)t));
        }
}

// lane k behind the wave_lds_sync that follows the last match_post: detection k's winner
struct MatchWinner {
    bool matched;
    unsigned l;       // the landmark (0 where nothing matched)
    unsigned mbits;   // the bits of its m: +0 where it was -0
};
__device__ __forceinline__ MatchWinner match_winner(const u64* s_best, unsigned lane, unsigned K)
{
    const u64 won = s_best[lane];
    MatchWinner w;
    w.matched = lane < K && won != ~0ull;
    w.l = w.matched ? (unsigned)won : 0u;
    w.mbits = (unsigned)(won >> 32);
    return w;
}

// f. row i of the table (rows of `stride` bytes): [0, rowb) from LDS (255 from L on), the rest of the stride 255
__device__ __forceinline__ void match_row_write(const unsigned char* s_row, unsigned rowb, uint8_t* table, int i, unsigned stride, unsigned lane)
{
    uint8_t* out = table + (size_t)i * stride;
    if ((stride & 3u) == 0 && (reinterpret_cast<uintptr_t>(table) & 3u) == 0) {   // (kernel-uniform) every row starts on a dword
        const unsigned* s_row32 = reinterpret_cast<const unsigned*>(s_row);
        unsigned* out32 = reinterpret_cast<unsigned*>(out);
        for (unsigned d = lane; d < stride / 4u; d += 64u) out32[d] = d < rowb / 4u ? s_row32[d] : 0xffffffffu;
    } else {
        for (unsigned c = lane; c < stride; c += 64u) out[c] = c < rowb ? s_row[c] : (uint8_t)255;
    }
}

}  // namespace slam
