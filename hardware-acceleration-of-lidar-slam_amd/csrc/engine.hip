// engine.hip — the engine handle behind the C ABI declared in include/slam_hip.h: errors and status strings, its life cycle
// and stream, HIP-event profiling, the self-test and the one bounded wait on a word in mapped host memory.  The stages are
// implemented in engine_match.hip, engine_ekf.hip, engine_assoc.hip and engine_resample.hip.
//
// The engine owns what the reference keeps in file-scope globals — the two occupancy/EDT grids
// (`occ_grid`, Subsystem_1/main.c:200-213), the current scan (`scan`, main.c:60-69) and the matcher
// result scratch (`FastMatchParameters`, main.c:374-379) — but as device-resident buffers behind an
// opaque handle, the shape of the `accel` handle of the reference's FPGA variant
// (Submodule_2/Hadrware_acclereated.cpp:842-845).  There is no CPU fallback anywhere in these files.

#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "comm.h"
#include "engine_internal.h"

using namespace slam;

// ---- shared with the other translation units (C++ linkage, declared in engine_internal.h)
int slam_engine_fail_hip(slam_engine* e, hipError_t err, const char* what)
{
    if (e) snprintf(e->err, sizeof e->err, "%s: %s", what, hipGetErrorString(err));
    (void)hipGetLastError();   // clear the sticky error so later calls can proceed
    return SLAM_ERR_HIP;
}

int slam_engine_wait_flag(slam_engine* e, slam_comm* comm, const volatile uint32_t* flag, uint32_t seq, const char* what)
{
    if (comm) return comm_wait_flag(comm, flag, seq);   // sharded: the word sits behind collectives
    if (slam_spin_flag(flag, seq)) return SLAM_OK;
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));   // the launch failed or the device is wedged: let the runtime tell us
    if (__atomic_load_n(flag, __ATOMIC_ACQUIRE) != seq) return slam_engine_fail_hip(e, hipErrorUnknown, what);
    return SLAM_OK;
}

// Every pinned host buffer of the engine comes out of ONE allocation (mapped into the device): an allocation of pinned host
// memory is answered by the driver some 10-50 ms later with a 65-80 ms hold of the process's queues (DESIGN.md section 8,
// profiles/r03_stall_trigger.txt), so the engine makes one, when it is created, instead of eight.
static hipError_t engine_host_block(slam_engine* e)
{
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_fm = up(sizeof(float) * (kFmIn + kFmOut + 4 + kFmPair)), b_plan = up(sizeof(int32_t) * (SLAM_PLAN_WORDS(kMaxRanks) + 1)),
                 b_small = 256, b_res = 1024, b_stage = up(sizeof(float) * kStageSlots * kStageFloats);
    const size_t total = b_fm + b_plan + 4 * b_small + b_res + b_stage;
    hipError_t err = hipHostMalloc(&e->h_block, total, hipHostMallocMapped);
    if (err != hipSuccess) return err;
    void* dblock = nullptr;
    if ((err = hipHostGetDevicePointer(&dblock, e->h_block, 0)) != hipSuccess) return err;
    char *h = static_cast<char*>(e->h_block), *d = static_cast<char*>(dblock);
    size_t off = 0;
    auto take = [&](size_t bytes, auto*& hp, auto*& dp) {
        hp = reinterpret_cast<std::remove_reference_t<decltype(hp)>>(h + off);
        dp = reinterpret_cast<std::remove_reference_t<decltype(dp)>>(d + off);
        off += bytes;
    };
    take(b_fm, e->h_fm, e->d_hfm);
    take(b_plan, e->h_plan, e->d_hplan);
    take(b_small, e->h_gate, e->d_hgate);
    take(b_small, e->h_heads, e->d_hheads);
    take(b_small, e->h_obs, e->d_hobs);
    take(b_small, e->h_det, e->d_hdet);
    take(b_res, e->h_pf_res, e->d_hpf_res);
    e->h_stage = reinterpret_cast<float*>(h + off);
    memset(e->h_block, 0, total);
    return hipSuccess;
}

extern "C" {

int slam_abi_version(void) { return SLAM_ABI_VERSION; }

const char* slam_status_string(int status)
{
    switch (status) {
    case SLAM_OK: return "ok";
    case SLAM_ERR_NO_DEVICE: return "no usable gfx950 device";
    case SLAM_ERR_INVALID_ARG: return "invalid argument";
    case SLAM_ERR_HIP: return "HIP runtime error";
    case SLAM_ERR_NOT_READY: return "stage inputs not provided yet";
    case SLAM_ERR_CAPACITY: return "capacity exceeded";
    case SLAM_ERR_COMM: return "exchange between ranks failed";
    default: return "unknown status";
    }
}

// why the last slam_engine_create of this thread failed (there is no engine to ask then): slam_last_error(NULL)
static thread_local char g_create_err[256] = "";

const char* slam_last_error(const slam_engine* e) { return e ? e->err : g_create_err; }

int slam_engine_create(int device, slam_engine** out)
{
    if (!out) return SLAM_ERR_INVALID_ARG;
    *out = nullptr;
    int ndev = 0;
    g_create_err[0] = 0;
    hipError_t herr = hipGetDeviceCount(&ndev);
    if (herr != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
        snprintf(g_create_err, sizeof g_create_err, "device %d of %d (hipGetDeviceCount: %s)", device, ndev, hipGetErrorString(herr));
        (void)hipGetLastError();
        return SLAM_ERR_NO_DEVICE;
    }
    hipDeviceProp_t prop;
    if ((herr = hipSetDevice(device)) != hipSuccess || (herr = hipGetDeviceProperties(&prop, device)) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err, "hipSetDevice / hipGetDeviceProperties(%d): %s", device, hipGetErrorString(herr));
        (void)hipGetLastError();
        return SLAM_ERR_NO_DEVICE;
    }
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {   // code objects are gfx950-only
        snprintf(g_create_err, sizeof g_create_err, "device %d is %s, not gfx950", device, prop.gcnArchName);
        return SLAM_ERR_NO_DEVICE;
    }
    slam_engine* e = new (std::nothrow) slam_engine();
    if (!e) return SLAM_ERR_HIP;
    e->device = device;
    if (const char* sr = getenv("SLAM_SURVIVOR_ROWS")) e->survivor_rows = atoi(sr) != 0;
    if (hipStreamCreateWithFlags(&e->own_stream, hipStreamNonBlocking) != hipSuccess ||
        e->fm_buf.ensure(sizeof(float) * (kFmIn + kFmOut)) != hipSuccess ||
        e->fm_work.ensure(sizeof(float) * 2 * kLattice * SLAM_MAX_BEAMS) != hipSuccess ||   // (the hits of two sweeps: the chained pair)
        engine_host_block(e) != hipSuccess ||
        e->gate_buf.ensure(kGateBufWords * sizeof(int32_t)) != hipSuccess ||   // flag | ticket | accumulators: see kernels.h
        e->heads_buf.ensure(2 * sizeof(int32_t)) != hipSuccess ||
        hipMemset(e->heads_buf.p, 0, 2 * sizeof(int32_t)) != hipSuccess ||   // the gate's flag + the ticket word of quantise_scan_kernel
        e->scan_buf.ensure(sizeof(float) * 2 * SLAM_MAX_BEAMS) != hipSuccess) {
        snprintf(g_create_err, sizeof g_create_err, "allocating the engine's buffers on device %d: %s", device,
                 hipGetErrorString(hipGetLastError()));
        slam_engine_destroy(e);
        return SLAM_ERR_NO_DEVICE;
    }
    e->h_gate[0] = 1;
    e->h_gate[1] = 0;
    e->h_heads[0] = 0;
    e->h_heads[1] = -1;   // nothing known yet
    e->h_obs[0] = 0;
    e->h_obs[1] = -1;
    {
        const int32_t one[kGateBufWords] = { 1 };   // "the previous frame resampled": nothing is carried into the first frame; the rest 0
        if (hipMemcpy(e->gate_buf.p, one, sizeof one, hipMemcpyHostToDevice) != hipSuccess) {
            (void)hipGetLastError();
            slam_engine_destroy(e);
            return SLAM_ERR_NO_DEVICE;
        }
    }
    e->stream = e->own_stream;
    *out = e;
    return SLAM_OK;
}

int slam_engine_destroy(slam_engine* e)
{
    if (!e) return SLAM_OK;
    (void)hipSetDevice(e->device);
    (void)hipStreamSynchronize(e->stream);
    for (auto& g : e->grid) {
        g.occ_buf.release();
        g.edt_buf.release();
        g.packed_buf.release();
        g.table_buf.release();
    }
    e->scan_buf.release();
    e->obs_buf.release();
    e->det_buf.release();
    e->sight_buf.release();
    e->fm_buf.release();
    e->fm_work.release();
    e->scratch.release();
    e->bmax_buf.release();
    e->scan_state.release();
    e->ll_buf.release();
    e->shard_buf.release();
    e->first_buf.release();
    for (auto& ev : e->stage_ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto& b : e->host_io) b.release();
    for (auto& pool : e->prof_pool)
        for (auto& p : pool) {
            (void)hipEventDestroy(p.start);
            (void)hipEventDestroy(p.stop);
        }
    if (e->h_block) (void)hipHostFree(e->h_block);   // every pinned buffer of the engine at once
    e->obs_list.release();
    e->heads_buf.release();
    e->gate_buf.release();
    e->carry_buf.release();
    e->spread_buf.release();
    e->modes_buf.release();
    e->reseed_buf.release();
    e->reseed_pair_buf.release();
    if (e->own_stream) (void)hipStreamDestroy(e->own_stream);
    delete e;
    return SLAM_OK;
}

int slam_profile_enable(slam_engine* e, int mask)
{
    SLAM_ENTER(e);
    e->prof_mask = mask;
    return SLAM_OK;
}

int slam_profile_read(slam_engine* e, int kernel, double* total_ms, int64_t* launches)
{
    SLAM_ENTER(e);
    if (kernel < 0 || kernel >= SLAM_PROF_COUNT || !total_ms || !launches) return SLAM_ERR_INVALID_ARG;
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    double sum = 0.0;
    for (size_t i = 0; i < e->prof_used[kernel]; ++i) {
        float ms = 0.0f;
        SLAM_HIP_TRY(e, hipEventElapsedTime(&ms, e->prof_pool[kernel][i].start, e->prof_pool[kernel][i].stop));
        sum += (double)ms;
    }
    *total_ms = sum;
    *launches = (int64_t)e->prof_used[kernel];
    e->prof_used[kernel] = 0;
    return SLAM_OK;
}

int slam_profile_bracket_overhead(slam_engine* e, double* overhead_ms)
{
    SLAM_ENTER(e);
    if (!overhead_ms) return SLAM_ERR_INVALID_ARG;
    enum { kPairs = 64 };
    hipEvent_t ev[2 * kPairs];
    for (auto& x : ev) SLAM_HIP_TRY(e, hipEventCreate(&x));
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    for (int k = 0; k < kPairs; ++k) {
        SLAM_HIP_TRY(e, hipEventRecord(ev[2 * k], e->stream));
        SLAM_HIP_TRY(e, hipEventRecord(ev[2 * k + 1], e->stream));
    }
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    double sum = 0.0;
    for (int k = 0; k < kPairs; ++k) {
        float ms = 0.0f;
        SLAM_HIP_TRY(e, hipEventElapsedTime(&ms, ev[2 * k], ev[2 * k + 1]));
        sum += (double)ms;
    }
    for (auto& x : ev) (void)hipEventDestroy(x);
    *overhead_ms = sum / kPairs;
    return SLAM_OK;
}

int slam_profile_copy_ceiling(slam_engine* e, const float* d_src, float* d_dst, int64_t rows, int plane_stride, int reps,
                              double* ms_per_copy)
{
    SLAM_ENTER(e);
    if (!d_src || !d_dst || d_src == d_dst || rows <= 0 || rows > 0x7fffffff || plane_stride < 128 || plane_stride % 128 ||
        reps <= 0 || !ms_per_copy)
        return SLAM_ERR_INVALID_ARG;
    hipEvent_t a, b;
    SLAM_HIP_TRY(e, hipEventCreate(&a));
    SLAM_HIP_TRY(e, hipEventCreate(&b));
    int rc = SLAM_OK;
    auto ok = [&](hipError_t err, const char* what) {
        if (err != hipSuccess && rc == SLAM_OK) rc = slam_engine_fail_hip(e, err, what);
        return err == hipSuccess;
    };
    for (int r = 0; r < 2 && rc == SLAM_OK; ++r) ok(launch_copy_rows(e->stream, d_src, d_dst, (int)rows, plane_stride), "copy_rows");
    ok(hipEventRecord(a, e->stream), "hipEventRecord");
    for (int r = 0; r < reps && rc == SLAM_OK; ++r) ok(launch_copy_rows(e->stream, d_src, d_dst, (int)rows, plane_stride), "copy_rows");
    ok(hipEventRecord(b, e->stream), "hipEventRecord");
    ok(hipEventSynchronize(b), "hipEventSynchronize");
    float ms = 0.0f;
    if (rc == SLAM_OK) ok(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime");
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    *ms_per_copy = (double)ms / reps;
    return rc;
}

int slam_selftest_reciprocal(slam_engine* e, int64_t* mismatches, int64_t* checked)
{
    SLAM_ENTER(e);
    if (!mismatches || !checked) return SLAM_ERR_INVALID_ARG;
    unsigned long long* d = nullptr;
    SLAM_HIP_TRY(e, hipMalloc((void**)&d, 16));
    int rc = SLAM_OK;
    unsigned long long h[2] = { 0, 0 };
    hipError_t err = hipMemsetAsync(d, 0, 16, e->stream);
    if (err == hipSuccess) err = launch_selftest_reciprocal(e->stream, d);
    if (err == hipSuccess) err = hipMemcpyAsync(h, d, 16, hipMemcpyDeviceToHost, e->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(e->stream);
    if (err != hipSuccess) rc = slam_engine_fail_hip(e, err, "slam_selftest_reciprocal");
    (void)hipFree(d);
    *mismatches = (int64_t)h[0];
    *checked = (int64_t)h[1];
    return rc;
}

int slam_engine_set_stream(slam_engine* e, void* hip_stream)
{
    SLAM_ENTER(e);
    e->stream = hip_stream == SLAM_OWN_STREAM ? e->own_stream : static_cast<hipStream_t>(hip_stream);
    return SLAM_OK;
}

int slam_engine_sync(slam_engine* e)
{
    SLAM_ENTER(e);
    SLAM_HIP_TRY(e, hipStreamSynchronize(e->stream));
    return SLAM_OK;
}

}  // extern "C"
