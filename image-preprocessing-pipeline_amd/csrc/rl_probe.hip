// Measurement entries of the RL context: what the experiments under profiles/ and the tests of the timing interface call to time
// single passes, the overlap of a split x pass with a stand-in collective, and the plan-time placement trial.  No product path
// calls any of them.
#include <chrono>

#include "rl_internal.h"

using namespace mi;

// A stand-in for a collective's kernels: `busy_wgs` small work-groups that hold their compute units for `ticks` of the 100-MHz
// wall clock (and touch `buf` so that they are not optimised away)
__global__ __launch_bounds__(256) void k_busy(long long ticks, int* __restrict__ buf) {
    extern __shared__ int hold[];  // (dynamic LDS: what keeps a 140-KB work-group of the x pass off this compute unit)
    hold[threadIdx.x] = (int)threadIdx.x;
    const long long t0 = wall_clock64();
    int spins = 0;
    while (wall_clock64() - t0 < ticks) {
        __builtin_amdgcn_s_sleep(32);
        ++spins;
    }
    if (threadIdx.x == 0 && buf) buf[blockIdx.x] = spins + hold[(spins + 1) & 255];
}

extern "C" int mi_rl_overlap_probe(mi_rl_ctx* ctx, void* stream, float* bl, const int* edge_rows, int busy_wgs, float busy_us, int reps,
                                   float* out_ms) {
    NativeFft* nf = nullptr;
    MI_TRY(sharded_native(ctx, &nf));
    MI_REQUIRE(bl && edge_rows && out_ms && reps > 0 && busy_wgs >= 0 && busy_wgs <= 1024 && busy_us >= 0.0f && busy_us <= 50000.0f,
               "mi_rl_overlap_probe: bad arguments");
    MI_REQUIRE(nf->splits(), "mi_rl_overlap_probe: this context cannot split the x pass");
    hipStream_t s = as_stream(stream), side = nullptr;
    const TileSelect sel = nf->edge_tiles(2, edge_rows[0], edge_rows[1], edge_rows[2], edge_rows[3]);
    ConvEpilogue e;
    e.a = bl;
    DevBuf sink;
    MI_TRY(sink.alloc(sizeof(int) * 1024));
    MI_HIP(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    hipEvent_t ev[4];
    for (auto& x : ev) MI_HIP(hipEventCreate(&x));
    int rc = MI_OK;
    float sum_x = 0.0f, sum_all = 0.0f;
    for (int r = -1; r < reps && rc == MI_OK; ++r) {  // r == -1: warm-up
        (void)hipStreamSynchronize(s);
        (void)hipEventRecord(ev[0], s);
        if (busy_wgs > 0) {
            (void)hipStreamWaitEvent(side, ev[0], 0);
            // 48 KB of LDS per stand-in work-group: it cannot share a compute unit with a work-group of the x pass (~140 of 160 KB),
            // like a collective's kernel with its staging buffers (a stand-in without LDS simply co-resides: measured, no effect)
            hipLaunchKernelGGL(k_busy, dim3((unsigned)busy_wgs), dim3(256), 48 * 1024, side, (long long)(busy_us * 100.0f), sink.as<int>());
            rc = launch_check("k_busy");
            (void)hipEventRecord(ev[3], side);
            // the stand-in must be resident before the pass is launched, like a collective that was issued first
            const auto t0 = std::chrono::steady_clock::now();
            while (std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count() < 150.0) {}
        }
        (void)hipEventRecord(ev[1], s);
        if (rc == MI_OK) rc = nf->x_inverse(s, nullptr, EPI_RATIO, e, true, &sel);
        (void)hipEventRecord(ev[2], s);
        if (busy_wgs > 0) (void)hipStreamWaitEvent(s, ev[3], 0);
        (void)hipEventRecord(ev[3], s);
        hipError_t he = hipEventSynchronize(ev[3]);
        float a = 0.0f, b = 0.0f;
        if (he == hipSuccess) he = hipEventElapsedTime(&a, ev[1], ev[2]);
        if (he == hipSuccess) he = hipEventElapsedTime(&b, ev[0], ev[3]);
        if (rc == MI_OK && he != hipSuccess) rc = fail(MI_ERR_HIP, "mi_rl_overlap_probe: %s", hipGetErrorString(he));
        if (r >= 0) { sum_x += a; sum_all += b; }
    }
    (void)hipStreamSynchronize(side);
    for (auto& x : ev) (void)hipEventDestroy(x);
    (void)hipStreamDestroy(side);
    out_ms[0] = sum_x / (float)reps;    // launch -> end of the x launch (part 2)
    out_ms[1] = sum_all / (float)reps;  // stand-in issued -> both finished
    return rc;
}

extern "C" int mi_rl_time_pass(mi_rl_ctx* ctx, void* stream, int which, const float* bl, int reps, float* avg_ms) {
    MI_REQUIRE(ctx && bl && avg_ms, "mi_rl_time_pass: null pointer");
    MI_TRY(use_device(ctx->dev));
    NativeFft* nf = native_of(ctx);
    if (!nf || ctx->fft->padded) return fail(MI_ERR_UNSUPPORTED, "mi_rl_time_pass: only the unpadded native FFT pipeline exposes its passes");
    return nf->time_pass(as_stream(stream), which, bl, reps, avg_ms);
}

extern "C" int mi_rl_time_between(mi_rl_ctx* ctx, void* stream, int which, const void* src, void* dst, float* bl, int reps, float* avg_ms) {
    MI_REQUIRE(ctx && src && dst && avg_ms && reps > 0 && (which == 0 || which == 3 || which == 4 || ((which == 1 || which == 2) && bl)), "mi_rl_time_between: bad arguments");
    MI_TRY(use_device(ctx->dev));
    NativeFft* nf = native_of(ctx);
    if (!nf || ctx->fft->padded) return fail(MI_ERR_UNSUPPORTED, "mi_rl_time_between: only the unpadded native FFT pipeline");
    return nf->time_between(as_stream(stream), which, static_cast<const float2*>(src), static_cast<float2*>(dst), bl, reps, avg_ms);
}

extern "C" int mi_rl_fft_placement(mi_rl_ctx* ctx, float* cost_ms, int cap, int* n, int* kept) {
    MI_REQUIRE(ctx && n && kept && (cost_ms || cap <= 0), "mi_rl_fft_placement: null pointer");
    *n = 0;
    *kept = -1;
    const NativeFft* nf = native_of(ctx);
    if (!nf) return MI_OK;
    const auto& ms = nf->place.placement_ms;
    *n = (int)ms.size();
    *kept = nf->place.placement_kept;
    for (int i = 0; i < *n && i < cap; ++i) cost_ms[i] = ms[i];
    return MI_OK;
}
