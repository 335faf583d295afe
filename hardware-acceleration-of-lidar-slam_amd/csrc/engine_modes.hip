// engine_modes.hip — the modes of a pose population on the engine (slam_pose_modes_dev; slam_pf_modes calls the same two steps):
// the parameters' checks, the buffers (made by the first call, kept zeroed by the select launch), the three launches of
// modes_kernels.hip, and the host arithmetic from the raw integer words to slam_pf_mode (specification: tests/_modes_spec.py).

#include <float.h>
#include <math.h>
#include <stdio.h>

#include "engine_internal.h"

using namespace slam;

namespace {

// bytes of the engine's modes buffer: the table | the list of claimed slots | the control words (64 bytes) | the raw result
constexpr size_t kTableBytes = sizeof(ModesCell) * (size_t)kModesSlots, kListBytes = sizeof(uint32_t) * (size_t)kModesSlots,
                 kCtrlBytes = 64, kRawBytes = sizeof(long long) * (size_t)kModesWords;
constexpr size_t kZeroedBytes = kTableBytes + kListBytes + kCtrlBytes, kBufBytes = kZeroedBytes + kRawBytes;

}  // namespace

int slam_engine_modes_launch(slam_engine* e, const float* d_x, const float* d_y, const float* d_theta, const int32_t* d_idx,
                             const float* d_carry, int n, float ref_theta, float cell, int hbins, int max_modes, long long* d_hout,
                             uint32_t* d_hseq, uint32_t seq, const long long** d_raw)
{
    if (n <= 0 || !d_x || !d_y || !d_theta) return SLAM_ERR_INVALID_ARG;
    if (!(cell > 0.0f && cell <= FLT_MAX) || !(hbins == 1 || (hbins >= 4 && hbins <= 64)) || max_modes < 1 || max_modes > kModesMax) {
        snprintf(e->err, sizeof e->err, "modes: cell must be finite and > 0, hbins 1 or 4 .. 64, max_modes 1 .. %d", kModesMax);
        return SLAM_ERR_INVALID_ARG;
    }
    if (!e->modes_cus) SLAM_HIP_TRY(e, hipDeviceGetAttribute(&e->modes_cus, hipDeviceAttributeMultiprocessorCount, e->device));
    if (!e->modes_buf.p) {
        SLAM_HIP_TRY(e, e->modes_buf.ensure(kBufBytes));
        e->modes_clean = false;
    }
    unsigned char* base = e->modes_buf.as<unsigned char>();
    if (!e->modes_clean) SLAM_HIP_TRY(e, hipMemsetAsync(base, 0, kZeroedBytes, e->stream));
    e->modes_clean = false;   // (until the three launches are out)
    ModesArgs a{};
    a.x = d_x;
    a.y = d_y;
    a.th = d_theta;
    a.idx = d_idx;
    a.carry = d_carry;
    a.n = n;
    a.ref_theta = ref_theta;
    a.inv_cell = 1.0f / cell;
    a.hbins = hbins;
    a.max_modes = max_modes;
    a.table = reinterpret_cast<ModesCell*>(base);
    a.list = reinterpret_cast<uint32_t*>(base + kTableBytes);
    a.ctrl = reinterpret_cast<unsigned long long*>(base + kTableBytes + kListBytes);
    a.out = reinterpret_cast<long long*>(base + kZeroedBytes);
    a.h_out = d_hout;
    a.h_seq = d_hseq;
    a.seq = seq;
    SLAM_HIP_TRY(e, launch_modes(e->stream, a, e->modes_cus));
    e->modes_clean = true;
    *d_raw = a.out;
    return SLAM_OK;
}

int slam_engine_modes_result(slam_engine* e, const long long* raw, float ref_theta, float cell, slam_pf_mode* modes, int* n_modes,
                             int* cells, int64_t* wtotal)
{
    if (raw[0] != 0) {
        snprintf(e->err, sizeof e->err, "modes: %lld particles lie outside the domain |x / cell|, |y / cell| < 2^20 with a finite heading "
                                        "(or are not numbers)", raw[0]);
        return SLAM_ERR_INVALID_ARG;
    }
    if (raw[1] > kModesMaxCells) {
        snprintf(e->err, sizeof e->err, "modes: the population occupies more than %d distinct cells: choose a larger cell or fewer heading bins",
                 kModesMaxCells);
        return SLAM_ERR_CAPACITY;
    }
    const long long wt = raw[2];
    const int count = (int)raw[3];
    for (int m = 0; m < count; ++m) {
        const long long* r = raw + kModesHead + kModesPer * m;
        const unsigned long long k = (unsigned long long)r[0] - 1ull;
        const int32_t c[3] = { (int32_t)(k >> 27) - (1 << 20), (int32_t)((k >> 6) & 0x1fffffull) - (1 << 20), (int32_t)(k & 63ull) };
        const long long wm = r[2];
        slam_pf_mode& o = modes[m];
        for (int ax = 0; ax < 2; ++ax) {
            const long long q = r[3 + ax] / wm;   // C's division truncates
            o.pose[ax] = (float)(((double)c[ax] + (double)q / 1048576.0) * (double)cell);
        }
        o.pose[2] = (float)((double)ref_theta + atan2((double)r[5], (double)r[6]));
        o.mass = (float)((double)wm / (double)wt);
        for (int k3 = 0; k3 < 3; ++k3) o.cell[k3] = c[k3];
        o.ncells = (int32_t)r[1];
        o.weight = wm;
    }
    *n_modes = count;
    *cells = (int)raw[1];
    if (wtotal) *wtotal = wt;
    return SLAM_OK;
}

extern "C" {

int slam_pose_modes_dev(slam_engine* e, const float* d_x, const float* d_y, const float* d_theta, const int32_t* d_idx,
                        const float* d_carry, int n, float ref_theta, float cell, int hbins, int max_modes, slam_pf_mode* modes,
                        int* n_modes, int* cells, int64_t* wtotal)
{
    SLAM_ENTER(e);
    if (!modes || !n_modes || !cells || !wtotal) return SLAM_ERR_INVALID_ARG;
    long long raw[kModesWords];
    for (int pass = 0; pass < 2; ++pass) {
        const long long* d_raw = nullptr;
        if (int rc = slam_engine_modes_launch(e, d_x, d_y, d_theta, d_idx, pass == 0 ? d_carry : nullptr, n, ref_theta, cell, hbins,
                                              max_modes, nullptr, nullptr, 0, &d_raw))
            return rc;
        SLAM_HIP_TRY(e, hipMemcpyAsync(raw, d_raw, sizeof raw, hipMemcpyDeviceToHost, e->stream));
        SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
        if (!(d_carry && raw[0] == 0 && raw[2] == 0)) break;   // (no weight at all: the plain form, as slam_pose_spread_dev)
    }
    return slam_engine_modes_result(e, raw, ref_theta, cell, modes, n_modes, cells, wtotal);
}

}  // extern "C"
