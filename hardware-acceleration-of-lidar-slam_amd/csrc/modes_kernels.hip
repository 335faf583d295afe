// modes_kernels.hip — the modes of a pose population: the few heaviest clusters of the cloud on a grid of cells (ix, iy, heading
// bin), each with a pose and a mass, from exact integer sums (slam_pf_modes, slam_pose_modes_dev; specification:
// tests/_modes_spec.py).  Three launches on one stream, nothing of the population or of the table is copied:
//   1. modes_accumulate_kernel: one pass over the 12 B per particle (plus the carried log-weight where the weights are unequal)
//      into an open-addressing table in device memory, 64-bit compare-and-swap on the key, 64-bit integer adds on the five sums —
//      integers, so any order gives the same sums.  A settled cloud puts every particle into a handful of cells, so the kernel
//      combines before it touches memory: a wavefront serves its distinct keys one after another (ballot, lowest lane first, the
//      key handed over by readlane; the lanes that hold it reduce their five integers across the wave, the lowest carries the
//      result on), the carrying lanes add into a small table in LDS (64-bit LDS atomics), and the workgroup flushes that table once
//      at its end; what finds no place in LDS within kLdsProbes probes goes straight to memory.  Persistent workgroups.
//   2. modes_score_kernel: one thread per occupied cell (the list of claimed slots): W summed over the 27 (9) cells of its
//      neighbourhood by probing the table.
//   3. modes_select_kernel: one workgroup — max_modes rounds of a block arg-max over (score, key) under the eligibility rule, by KEY
//      and never by slot (the slot a key landed in depends on the schedule), the member sums of each centre, the hand-over to device
//      and mapped host memory behind a sequence number, and the claimed slots zeroed for the next call.
// 2 and 3 stay two launches: the score wants the machine (up to 65 536 cells x 26 probes), the selection is one workgroup by
// nature, and joining them needs either a last-workgroup ticket with the selection behind it or a grid-wide wait; the boundary
// costs a couple of microseconds and keeps both kernels plain.
// "More than kModesMaxCells distinct cells" is an exact count of successful key insertions: a thread claims an empty slot only
// while the count it reads is at most kModesMaxCells; once it is larger the verdict is settled (so many distinct keys exist) and
// what is dropped belongs to a refused call.  At most one claim per thread is between its look at the count and its add, so the
// count — and the table's load — never passes kModesMaxCells + 1 + (threads of the launch) < kModesSlots: every probe ends.

#include <float.h>

#include <type_traits>

#include "block_reduce.h"
#include "det_math.h"
#include "kernels.h"

namespace slam {
namespace {

using u64 = unsigned long long;

constexpr int kLdsCells = 256;     // of a workgroup's table in LDS: 6 x 8 B each, 12 KiB
constexpr int kLdsProbes = 4;
constexpr int kSelectBlock = 1024;
constexpr int kUBias = 1 << 20;    // ix, iy in [-2^20, 2^20)
static_assert(kModesMaxCells + 1 + kModesMaxBlocks * kBlock < kModesSlots, "the table must outlast every claim in flight");
static_assert((kModesSlots & (kModesSlots - 1)) == 0 && (kLdsCells & (kLdsCells - 1)) == 0, "powers of two");
static_assert(sizeof(ModesCell) == 64, "one cell, one 64-byte line");

__device__ __forceinline__ u64 pack_key(int ix, int iy, int b)
{
    return 1ull + (((u64)(uint32_t)(ix + kUBias) << 27) | ((u64)(uint32_t)(iy + kUBias) << 6) | (u64)(uint32_t)b);
}
__device__ __forceinline__ void unpack_key(u64 key, int& ix, int& iy, int& b)
{
    const u64 k = key - 1ull;
    ix = (int)(uint32_t)(k >> 27) - kUBias;
    iy = (int)(uint32_t)((k >> 6) & 0x1fffffull) - kUBias;
    b = (int)(uint32_t)(k & 63ull);
}
__device__ __forceinline__ uint32_t hash_key(u64 key) { return (uint32_t)((key * 0x9E3779B97F4A7C15ull) >> 40); }

__device__ __forceinline__ u64 wave_read(u64 v, int owner)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, owner),
                   hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), owner);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ u64 shfl_xor(u64 v, int o)
{
    const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
    return ((u64)hi << 32) | lo;
}
__device__ __forceinline__ int wave_sum(int v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) { return (long long)wave_sum_u64((uint64_t)v); }

// the cell of `key`, or nullptr (the table is not being written: launches 2 and 3)
__device__ __forceinline__ const ModesCell* find_cell(const ModesCell* __restrict__ table, u64 key)
{
    uint32_t h = hash_key(key) & (kModesSlots - 1);
    for (int p = 0; p < kModesSlots; ++p, h = (h + 1) & (kModesSlots - 1)) {
        const u64 k = table[h].key;
        if (k == key) return table + h;
        if (k == 0) return nullptr;
    }
    return nullptr;
}

// five sums into the cell of `key`, claimed on the way where it is new
__device__ __forceinline__ void table_add(const ModesArgs& a, u64 key, const u64 (&v)[5])
{
    unsigned int* count = reinterpret_cast<unsigned int*>(a.ctrl);
    uint32_t h = hash_key(key) & (kModesSlots - 1);
    for (int p = 0; p < kModesSlots; ++p, h = (h + 1) & (kModesSlots - 1)) {
        ModesCell* c = a.table + h;
        u64 k = __hip_atomic_load(&c->key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (k == 0) {
            if (__hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > (unsigned)kModesMaxCells) return;   // the verdict is settled
            k = atomicCAS(&c->key, 0ull, key);
            if (k == 0) {
                const uint32_t pos = atomicAdd(count, 1u);
                if (pos < (uint32_t)kModesSlots) a.list[pos] = h;
                k = key;
            }
        }
        if (k == key) {
#pragma unroll
            for (int j = 0; j < 5; ++j) atomicAdd(&c->sum[j], v[j]);
            return;
        }
    }
    atomicMax(count, (unsigned)kModesMaxCells + 1u);   // (never: the table outlasts every claim; refuse rather than lose a sum)
}

// COMBINE = false is the measurement form (a build with -DSLAM_MODES_NO_COMBINE, profiles/modes_probe.py): one set of memory
// atomics per particle
#ifdef SLAM_MODES_NO_COMBINE
constexpr bool kCombine = false;
#else
constexpr bool kCombine = true;
#endif
template <bool WEIGHTED, bool COMBINE>
__global__ __launch_bounds__(kBlock) void modes_accumulate_kernel(ModesArgs a)
{
    using T = std::conditional_t<WEIGHTED, long long, int>;   // a wavefront's sum of one key: 64 x 2^20 (x 2^16 where weighted)
    __shared__ u64 s_key[kLdsCells];
    __shared__ u64 s_sum[5][kLdsCells];
    __shared__ uint64_t s_red[kBlock / 64];
    if (COMBINE) {
        for (int i = threadIdx.x; i < kLdsCells; i += kBlock) {
            s_key[i] = 0;
#pragma unroll
            for (int j = 0; j < 5; ++j) s_sum[j][i] = 0;
        }
        __syncthreads();
    }
    const int lane = threadIdx.x & 63;
    uint32_t outside = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    // (the wavefront walks together: the loop's bounds are the same in all its lanes)
    for (int64_t base = (int64_t)blockIdx.x * kBlock + (threadIdx.x & ~63); base < a.n; base += stride) {
        const int64_t i = base + lane;
        bool active = false;
        u64 key = 0;
        T v[5] = { 0, 0, 0, 0, 0 };
        if (i < a.n) {
            const int64_t j = a.idx ? a.idx[i] : i;
            const float px = a.x[j], py = a.y[j], pt = a.th[j];
            const float ux = px * a.inv_cell, uy = py * a.inv_cell;
            const bool inside = fabsf(ux) < 1048576.0f && fabsf(uy) < 1048576.0f && fabsf(pt) <= FLT_MAX;   // (false for NaN)
            const uint32_t w = WEIGHTED ? (uint32_t)((uint64_t)(det_expf(a.carry[i]) * 4294967296.0f) >> 16) : 1u;
            if (!inside) {
                ++outside;
            } else if (w != 0) {
                const float flx = floorf(ux), fly = floorf(uy);
                const int fx = (int)((ux - flx) * 1048576.0f), fy = (int)((uy - fly) * 1048576.0f);
                float t = pt * 0.15915494f;
                t = t - floorf(t);
                const int b = min((int)(t * (float)a.hbins), a.hbins - 1);
                float s, c;
                det_sincosf(pt - a.ref_theta, s, c);
                const int si = (int)(s * 1048576.0f), ci = (int)(c * 1048576.0f);
                key = pack_key((int)flx, (int)fly, b);
                v[0] = (T)w;
                v[1] = (T)w * fx;
                v[2] = (T)w * fy;
                v[3] = (T)w * si;
                v[4] = (T)w * ci;
                active = true;
            }
        }
        if (COMBINE) {
            // the wavefront serves its distinct keys one after another, the lowest lane that still holds one first; everything at
            // the loop head is wave-uniform.  Behind the loop the active lanes are the owners: one per distinct key.
            for (u64 todo = __ballot(active); todo;) {
                const int owner = __ffsll(todo) - 1;
                const u64 okey = wave_read(key, owner);
                const bool mine = active && key == okey;
                const u64 holders = __ballot(mine);
                todo &= ~holders;
                if (__popcll(holders) > 1) {
#pragma unroll
                    for (int j = 0; j < 5; ++j) {
                        const T total = wave_sum(mine ? v[j] : (T)0);
                        if (lane == owner) v[j] = total;
                    }
                    if (mine && lane != owner) active = false;
                }
            }
        }
        if (active) {
            const u64 add[5] = { (u64)(long long)v[0], (u64)(long long)v[1], (u64)(long long)v[2], (u64)(long long)v[3], (u64)(long long)v[4] };
            bool placed = false;
            if (COMBINE) {
                uint32_t h = hash_key(key) & (kLdsCells - 1);
                for (int p = 0; p < kLdsProbes && !placed; ++p, h = (h + 1) & (kLdsCells - 1)) {
                    const u64 prev = atomicCAS(&s_key[h], 0ull, key);
                    if (prev == 0 || prev == key) {
#pragma unroll
                        for (int j = 0; j < 5; ++j) atomicAdd(&s_sum[j][h], add[j]);
                        placed = true;
                    }
                }
            }
            if (!placed) table_add(a, key, add);
        }
    }
    if (COMBINE) {
        __syncthreads();
        for (int i = threadIdx.x; i < kLdsCells; i += kBlock) {
            const u64 key = s_key[i];
            if (key == 0) continue;
            const u64 add[5] = { s_sum[0][i], s_sum[1][i], s_sum[2][i], s_sum[3][i], s_sum[4][i] };
            table_add(a, key, add);
        }
    }
    const uint64_t out_all = block_sum_u64<false>((uint64_t)outside, s_red);
    if (threadIdx.x == 0 && out_all != 0) atomicAdd(&a.ctrl[1], (u64)out_all);
}

__device__ __forceinline__ bool refused(const ModesArgs& a, uint32_t& count)
{
    count = *reinterpret_cast<const unsigned int*>(a.ctrl);
    return count > (uint32_t)kModesMaxCells || a.ctrl[1] != 0;
}

// the cells of the neighbourhood of (ix, iy, b), q = 0 .. 26: false where q names none (outside the grid; a heading step with one bin)
__device__ __forceinline__ bool neighbour_key(int ix, int iy, int b, int hbins, int q, u64& key, int& dx, int& dy)
{
    dx = q / 9 - 1;
    dy = (q / 3) % 3 - 1;
    const int db = q % 3 - 1;
    const int nx = ix + dx, ny = iy + dy;
    if ((hbins == 1 && db != 0) || nx < -kUBias || nx >= kUBias || ny < -kUBias || ny >= kUBias) return false;
    key = pack_key(nx, ny, (b + db + hbins) % hbins);   // (hbins >= 4: the three bins differ)
    return true;
}

__global__ __launch_bounds__(kBlock) void modes_score_kernel(ModesArgs a)
{
    __shared__ uint64_t s_red[kBlock / 64];
    uint32_t count;
    if (refused(a, count)) return;   // (the same in every thread)
    uint64_t wsum = 0;
    for (uint32_t i = blockIdx.x * kBlock + threadIdx.x; i < count; i += gridDim.x * kBlock) {
        ModesCell* c = a.table + a.list[i];
        int ix, iy, b;
        unpack_key(c->key, ix, iy, b);
        const u64 own = c->sum[0];
        u64 score = own;
        for (int q = 0; q < 27; ++q) {
            u64 key;
            int dx, dy;
            if (q == 13 || !neighbour_key(ix, iy, b, a.hbins, q, key, dx, dy)) continue;
            const ModesCell* nb = find_cell(a.table, key);
            if (nb) score += nb->sum[0];
        }
        c->score = score;
        wsum += own;
    }
    wsum = block_sum_u64<false>(wsum, s_red);
    if (threadIdx.x == 0 && wsum != 0) atomicAdd(&a.ctrl[2], (u64)wsum);
}

__device__ __forceinline__ int cyclic(int a, int b, int hbins)
{
    const int d = abs(a - b);
    return min(d, hbins - d);
}

__global__ __launch_bounds__(kSelectBlock) void modes_select_kernel(ModesArgs a)
{
    __shared__ u64 s_score[kSelectBlock / 64], s_bkey[kSelectBlock / 64];
    __shared__ u64 s_centre[kModesMax];
    __shared__ u64 s_acc[kModesMax][6];   // member cells, Wm, A_x, A_y, sum w S, sum w C
    __shared__ long long s_out[kModesWords];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint32_t count;
    const bool refuse = refused(a, count);
    const u64 outside = a.ctrl[1], wtotal = a.ctrl[2];
    for (int i = tid; i < kModesWords; i += kSelectBlock) s_out[i] = 0;
    for (int i = tid; i < kModesMax * 6; i += kSelectBlock) s_acc[i / 6][i % 6] = 0;
    int n_modes = 0;
    if (!refuse) {
        for (int r = 0; r < a.max_modes; ++r) {
            u64 best_s = 0, best_k = ~0ull;   // (an occupied cell scores its own W >= 1)
            for (uint32_t i = tid; i < count; i += kSelectBlock) {
                const ModesCell* c = a.table + a.list[i];
                const u64 k = c->key, sc = c->score;
                int ix, iy, b;
                unpack_key(k, ix, iy, b);
                bool eligible = true;
                for (int q = 0; q < r; ++q) {
                    int cx, cy, cb;
                    unpack_key(s_centre[q], cx, cy, cb);
                    if (abs(ix - cx) <= 2 && abs(iy - cy) <= 2 && cyclic(b, cb, a.hbins) <= 2) eligible = false;
                }
                if (eligible && (sc > best_s || (sc == best_s && k < best_k))) {
                    best_s = sc;
                    best_k = k;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const u64 os = shfl_xor(best_s, o), ok = shfl_xor(best_k, o);
                if (os > best_s || (os == best_s && ok < best_k)) {
                    best_s = os;
                    best_k = ok;
                }
            }
            if (lane == 0) {
                s_score[wave] = best_s;
                s_bkey[wave] = best_k;
            }
            __syncthreads();
            if (tid == 0) {
                for (int w = 1; w < kSelectBlock / 64; ++w)
                    if (s_score[w] > best_s || (s_score[w] == best_s && s_bkey[w] < best_k)) {
                        best_s = s_score[w];
                        best_k = s_bkey[w];
                    }
                s_centre[r] = best_s ? best_k : 0ull;
            }
            __syncthreads();
            if (s_centre[r] == 0) break;   // no eligible cell ends the list (the same in every thread)
            ++n_modes;
        }
        // the member sums: one thread per (centre, cell of its neighbourhood)
        if (tid < n_modes * 27) {
            const int m = tid / 27, q = tid % 27;
            int ix, iy, b, dx, dy;
            unpack_key(s_centre[m], ix, iy, b);
            u64 key;
            if (neighbour_key(ix, iy, b, a.hbins, q, key, dx, dy)) {
                const ModesCell* c = find_cell(a.table, key);
                if (c) {
                    const long long w = (long long)c->sum[0];
                    atomicAdd(&s_acc[m][0], 1ull);
                    atomicAdd(&s_acc[m][1], (u64)w);
                    atomicAdd(&s_acc[m][2], (u64)(w * dx * 1048576ll + (long long)c->sum[1]));
                    atomicAdd(&s_acc[m][3], (u64)(w * dy * 1048576ll + (long long)c->sum[2]));
                    atomicAdd(&s_acc[m][4], c->sum[3]);
                    atomicAdd(&s_acc[m][5], c->sum[4]);
                }
            }
        }
    }
    __syncthreads();   // (also: every thread has read ctrl and is done with the table)
    if (tid == 0) {
        s_out[0] = (long long)outside;
        s_out[1] = (long long)count;
        s_out[2] = (long long)wtotal;
        s_out[3] = n_modes;
    }
    if (tid < n_modes) {
        long long* o = s_out + kModesHead + kModesPer * tid;
        o[0] = (long long)s_centre[tid];
        for (int j = 0; j < 6; ++j) o[1 + j] = (long long)s_acc[tid][j];
    }
    __syncthreads();
    for (int i = tid; i < kModesWords; i += kSelectBlock) {
        a.out[i] = s_out[i];
        if (a.h_out) a.h_out[i] = s_out[i];
    }
    // the claimed slots back to zero: the table is all zero again behind this launch
    const uint32_t claimed = count < (uint32_t)kModesSlots ? count : (uint32_t)kModesSlots;
    for (uint32_t i = tid; i < claimed; i += kSelectBlock) {
        u64* c = reinterpret_cast<u64*>(a.table + a.list[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) c[j] = 0;
    }
    if (tid < 3) a.ctrl[tid] = 0;
    if (a.h_out) {
        __threadfence_system();
        __syncthreads();
        if (tid == 0) __hip_atomic_store(a.h_seq, a.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace

hipError_t launch_modes(hipStream_t stream, const ModesArgs& a, int cus)
{
    if (a.n <= 0) return hipErrorInvalidValue;
    // persistent workgroups, 2048 particles each before the grid fills the machine once: every workgroup ends on a flush of its
    // distinct cells, atomics to the same few lines when the cloud has settled, so fewer and longer workgroups win below that
    const int want = (int)(((int64_t)a.n + 2047) / 2048), cap = cus > 0 && cus < kModesMaxBlocks ? cus : kModesMaxBlocks;
    const int nb = want < cap ? want : cap;
    if (a.carry)
        modes_accumulate_kernel<true, kCombine><<<nb, kBlock, 0, stream>>>(a);
    else
        modes_accumulate_kernel<false, kCombine><<<nb, kBlock, 0, stream>>>(a);
    modes_score_kernel<<<64, kBlock, 0, stream>>>(a);
    modes_select_kernel<<<1, kSelectBlock, 0, stream>>>(a);
    return hipGetLastError();
}

}  // namespace slam
