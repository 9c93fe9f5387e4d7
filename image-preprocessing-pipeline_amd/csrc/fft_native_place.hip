// Where the spectrum arrays of a plan lie -- the placement trial of NativeFft::init and the settling of the spare S buffer on the
// first fused iterations -- and the event-timed single passes of the bench.
#include <mutex>

#include "fft_native.h"

namespace mi {

namespace {
thread_local int tl_no_placement_trial = 0;
}
NoPlacementTrial::NoPlacementTrial() { ++tl_no_placement_trial; }
NoPlacementTrial::~NoPlacementTrial() { --tl_no_placement_trial; }
bool NoPlacementTrial::active() { return tl_no_placement_trial != 0; }

// Where the spectrum arrays lie.  A strided pass runs at one of two speeds depending on the PHYSICAL memory behind the array
// it reads and the array it writes: K buffers of one array's size allocated side by side fall into groups (runs of ~32 GB on one
// box: the size of an HBM stack), and the forward y pass of C3 takes 3.10 ms between two buffers of one group, 2.98 ms across
// groups; the update launch of the x pass takes 6.1 instead of 5.5 ms when the array it writes shares a group with the volume
// (profiles/r04_spectrum_halves.txt).  Two arrays carved out of ONE allocation -- rounds 1-3 -- mostly share a group: the slow
// placement of those rounds, and what a fresh process' first allocation regularly gets.  So large arrays are placed by trial:
// up to MI_FFT_PLACE_CANDIDATES (6) buffers are allocated side by side (as many as the free memory allows beside 24 GB for the
// caller), the passes are timed on every ordered pair (S read by the four y passes, T read by the two z and the two x passes of
// an iteration: cost = 4 y(S -> T) + 3 update(T -> S), on a stand-in volume, contents do not matter), the best pair stays, the
// rest goes back to the driver.  ~0.5 s and, for a moment, the candidates' memory at plan creation; arrays of
// MI_FFT_PLACE_MIN_MB (6144, both together) and more -- smaller plans are not tried: decwrap creates its block plans, 3-4 GB
// each, on several workers per device while others compute, and every released candidate is a device-wide synchronisation
// (slab.SlabRL lowers the limit for its rank, which has its device to itself).
// `gap`: bytes between S and T in the single allocation of init, which stands when fewer than two candidates fit.
int NativeFft::place_by_trial(hipStream_t s, size_t gap) {
    const int Hx = dims.hx;
    const size_t n_buf = spec_bytes / sizeof(float2);
    int tries = sw.place_candidates;
    // one trial at a time per device (plans created concurrently -- decwrap's workers with a large --block-size-max -- would each
    // hold their candidates and push each other out of memory); what the pool keeps cached goes back to the driver first: the
    // candidates are allocated behind the pool's back and get none of its trim-on-failure
    static std::mutex trial_mu[16];
    int dev_id = 0;
    MI_HIP(hipGetDevice(&dev_id));
    std::lock_guard<std::mutex> trial_lock(trial_mu[dev_id & 15]);
    (void)mi_release_cached_memory(dev_id);
    size_t free_b = 0, total_b = 0;
    MI_HIP(hipMemGetInfo(&free_b, &total_b));
    const size_t vol_bytes = sizeof(float) * 2 * (size_t)Hx * dims.ny * dims.nz;
    const size_t half = sizeof(float2) * n_buf, keep = ((size_t)24 << 30) + vol_bytes;
    while (tries > 1 && (size_t)tries * half + keep > free_b) --tries;
    if (tries < 2) return MI_OK;   // (no room for candidates: the single allocation stands)
    struct TrialEvents {   // (destroyed on every path out of the trial)
        hipEvent_t a = nullptr, b = nullptr;
        ~TrialEvents() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } tev;
    MI_HIP(hipEventCreate(&tev.a));
    MI_HIP(hipEventCreate(&tev.b));
    const hipEvent_t e0 = tev.a, e1 = tev.b;
    (void)hipFree(S.p);   // (the single allocation made by init makes room for the candidates)
    S.p = nullptr;
    const size_t block_bytes = S.bytes;
    S.bytes = 0;
    t_spec = nullptr;
    void* xtmp = nullptr;
    if (hipMalloc(&xtmp, vol_bytes) != hipSuccess) { (void)hipGetLastError(); xtmp = nullptr; }
    std::vector<void*> cand;
    for (int i = 0; i < tries; ++i) {
        void* q = nullptr;
        if (hipMalloc(&q, half) != hipSuccess) { (void)hipGetLastError(); break; }
        cand.push_back(q);
    }
    const int K = (int)cand.size();
    int rc = MI_OK, bi = -1, bj = -1, kept_idx = -1;
    float best = 0.0f;
    std::vector<float> ms, tyv((size_t)K * K, 0.0f);
    auto timed = [&](auto&& launch, float* out) {   // (two launches, the second counts)
        for (int rep = 0; rep < 2 && rc == MI_OK; ++rep) {
            (void)hipEventRecord(e0, s);
            rc = launch();
            (void)hipEventRecord(e1, s);
            if (rc == MI_OK && hipEventSynchronize(e1) != hipSuccess) rc = fail(MI_ERR_HIP, "native FFT: placement trial failed");
            if (rc == MI_OK) (void)hipEventElapsedTime(out, e0, e1);
        }
    };
    for (int i = 0; i < K && rc == MI_OK; ++i)
        for (int j = 0; j < K && rc == MI_OK; ++j) {
            if (i == j) continue;
            S.p = cand[i];
            t_spec = static_cast<float2*>(cand[j]);
            float ty = 0.0f, tx = 0.0f;
            timed([&] { return y_pass(s, false, y_route(dims)); }, &ty);
            if (xtmp) {
                ConvEpilogue ep;
                ep.a = static_cast<const float*>(xtmp);
                timed([&] { return x_inverse(s, static_cast<float*>(xtmp), EPI_UPDATE, ep, true); }, &tx);
            }
            tyv[(size_t)i * K + j] = ty;
            const float cost = 4.0f * ty + 3.0f * tx;
            if (bi < 0 || cost < best) { best = cost; bi = i; bj = j; kept_idx = (int)ms.size(); }
            ms.push_back(cost);
        }
    if (xtmp) (void)hipFree(xtmp);
    // a second buffer for S stays until the first call that brings the caller's volume: the update launch is slow when S
    // shares a region with THAT volume, which nothing here can know (NativeFft::iterate settles it: settle_s)
    int bk = -1;
    if (rc == MI_OK && bi >= 0 && half >= sw.alt_min)   // (MI_FFT_PLACE_ALT_MIN_MB: the smallest array that keeps a second buffer for S)
        for (int k = 0; k < K; ++k)
            if (k != bi && k != bj && tyv[(size_t)k * K + bj] <= 1.03f * tyv[(size_t)bi * K + bj] + 0.02f &&
                (bk < 0 || tyv[(size_t)k * K + bj] < tyv[(size_t)bk * K + bj]))
                bk = k;
    for (int i = 0; i < K; ++i)
        if (rc != MI_OK || bi < 0 || (i != bi && i != bj && i != bk)) (void)hipFree(cand[i]);
    if (bk >= 0) { place.S_alt.p = cand[bk]; place.S_alt.bytes = half; }
    S.p = nullptr;
    t_spec = nullptr;
    if (rc != MI_OK) return rc;
    if (bi < 0) {   // (fewer than two candidates: back to the single allocation)
        MI_TRY(S.alloc(block_bytes));
        t_spec = S.as<float2>() + n_buf + gap / sizeof(float2);
    } else {
        S.p = cand[bi];
        S.bytes = half;
        place.T2.p = cand[bj];
        place.T2.bytes = half;
        t_spec = place.T2.as<float2>();
        place.placement_ms = ms;
        place.placement_kept = kept_idx;   // (index in the list of ordered pairs (i, j), i != j, i slowest)
        if (sw.place_log) {   // (MI_FFT_PLACE_LOG: diagnostics on stderr)
            float worst = best;
            for (float v : ms) worst = std::max(worst, v);
            std::fprintf(stderr, "native FFT: 2 x %.1f GB placed on buffers %d (S) and %d (T) of %d: 4 y + 3 update %.2f ms (pairs from %.2f to %.2f)\n",
                         (double)half / 1e9, bi, bj, K, (double)best, (double)best, (double)worst);
        }
    }
    return MI_OK;
}

// Which of the two buffers kept for S goes with the CALLER's volume is settled on the first update launches of the fused loop
// themselves: the update launch is slow when the array it writes shares a memory region with the volume it rewrites, and only
// that launch shows it (the ratio launch and the forward x pass, which only read the volume, do not).  The first update launch
// that is followed by another iteration is timed writing the first buffer, the second one writing the other buffer -- every x
// launch writes S completely and the passes before it have consumed the old contents, so the buffer can change from one x launch
// to the next -- and the next x launch already goes to the faster of the two; the loser returns to the driver.
void NativeFft::settle_before_update() {
    if (place.alt_phase == 1) std::swap(S.p, place.S_alt.p);   // (the second buffer's turn)
}

int NativeFft::settle_decide(hipStream_t s) {
    (void)s;
    float t[2] = {0.0f, 0.0f};
    hipError_t he = hipEventSynchronize(place.alt_ev[3]);
    if (he == hipSuccess) he = hipEventElapsedTime(&t[0], place.alt_ev[0], place.alt_ev[1]);
    if (he == hipSuccess) he = hipEventElapsedTime(&t[1], place.alt_ev[2], place.alt_ev[3]);
    for (auto& e : place.alt_ev) { (void)hipEventDestroy(e); e = nullptr; }
    // now S.p is the second buffer, place.S_alt.p the first
    if (he != hipSuccess || t[0] <= 1.02f * t[1]) std::swap(S.p, place.S_alt.p);
    if (sw.place_log)
        std::fprintf(stderr, "native FFT: S settled on the %s buffer (update launch %.3f / %.3f ms with this volume)\n",
                     (he != hipSuccess || t[0] <= 1.02f * t[1]) ? "first" : "second", (double)t[0], (double)t[1]);
    (void)hipFree(place.S_alt.p);   // (waits for the device: the passes that still read it have run by then)
    place.S_alt.p = nullptr;
    place.S_alt.bytes = 0;
    place.alt_phase = 3;
    return he == hipSuccess ? MI_OK : fail(MI_ERR_HIP, "native FFT: settling S: %s", hipGetErrorString(he));
}

int NativeFft::release_spare() {
    if (!place.S_alt.p || place.alt_phase >= 3) return MI_OK;
    if (place.alt_phase == 2) return settle_decide(nullptr);   // (both update launches have been timed: keep the faster buffer)
    // phase 0 / 1: S.p is the first buffer, the second was never (or not yet) written by a launch whose output is still needed
    for (auto& e : place.alt_ev)
        if (e) { (void)hipEventDestroy(e); e = nullptr; }
    (void)hipFree(place.S_alt.p);   // (waits for the device)
    place.S_alt.p = nullptr;
    place.S_alt.bytes = 0;
    place.alt_phase = 3;
    return MI_OK;
}

// `reps` launches behind a warm-up launch between two events on `s`: their average duration in ms (`who`: for the failure message)
template <class F>
static int timed_launches(hipStream_t s, int reps, const char* who, float* avg_ms, F&& launch) {
    struct Events {   // (destroyed on every path)
        hipEvent_t a = nullptr, b = nullptr;
        ~Events() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    } ev;
    MI_HIP(hipEventCreate(&ev.a));
    MI_HIP(hipEventCreate(&ev.b));
    int rc = MI_OK;
    for (int r = -1; r < reps && rc == MI_OK; ++r) {  // r == -1: warm-up launch
        if (r == 0) (void)hipEventRecord(ev.a, s);
        rc = launch();
    }
    (void)hipEventRecord(ev.b, s);
    hipError_t he = hipEventSynchronize(ev.b);
    float ms = 0.0f;
    if (he == hipSuccess) he = hipEventElapsedTime(&ms, ev.a, ev.b);
    if (rc == MI_OK && he != hipSuccess) rc = fail(MI_ERR_HIP, "%s: %s", who, hipGetErrorString(he));
    *avg_ms = ms / (float)reps;
    return rc;
}

// Average duration (ms) of one launch of a single pass, measured with HIP events on `s` (bench.py's roofline leg).
// which: 0 x forward, 1 y forward, 2 z convolution, 3 y inverse, 4 fused x inverse+ratio+forward, 5 fused x inverse+update+
// forward (this one overwrites bl with |bl .* c| of whatever the buffers hold).  The buffers
// keep whatever the previous convolution left in them; `bl` is only read.
int NativeFft::time_pass(hipStream_t s, int which, const float* bl, int reps, float* avg_ms) {
    MI_REQUIRE(reps > 0 && avg_ms && which >= 0 && which <= 5, "time_pass: bad arguments");
    ConvEpilogue e;
    e.a = bl;
    return timed_launches(s, reps, "time_pass", avg_ms, [&] {
        switch (which) {
            case 0: return x_forward(s, bl);
            case 4: return x_inverse(s, nullptr, EPI_RATIO, e, true);
            case 5: return x_inverse(s, const_cast<float*>(bl), EPI_UPDATE, e, true);
            // (blocked middle: the whole chain is quoted as pass 1, passes 2 and 3 do not exist on their own)
            case 1: return y_pass(s, false, y_route(dims));
            case 2: return z_conv(s, false);
            default: return y_pass(s, true, y_route(dims));
        }
    });
}

// the same between two caller buffers standing in for the plan's arrays: which 0 forward y pass src -> dst, 2 forward x pass bl -> dst,
// 3 z pass src -> dst, 4 z pass on the plan's arrays with `src` as the (real) OTF, else the update launch src -> bl, dst
int NativeFft::time_between(hipStream_t s, int which, const float2* src, float2* dst, float* bl, int reps, float* avg_ms) {
    void* const s_own = S.p;
    float2* const t_own = t_spec;
    ConvEpilogue ep;
    ep.a = bl;
    return timed_launches(s, reps, "time_between", avg_ms, [&] {
        int rc;
        if (which == 0) {
            rc = y_pass(s, false, y_route(dims), src, dst);
        } else if (which == 2) {   // the forward x pass reads the volume and writes S
            S.p = dst;
            rc = x_forward(s, bl);
            S.p = s_own;
        } else if (which == 3) {   // the z pass reads T (and the OTF), writes S
            rc = z_conv(s, false, src, dst);
        } else if (which == 4) {   // the z pass on the context's own arrays with `src` standing in for the (real) OTF
            void* const g_own = Gr.p;
            if (!g_own) return fail(MI_ERR_UNSUPPORTED, "time_between: no real OTF");
            Gr.p = const_cast<float2*>(src);
            rc = z_conv(s, false);
            Gr.p = g_own;
        } else {   // the update launch reads T and writes S: the two buffers stand in for them
            t_spec = const_cast<float2*>(src);
            S.p = dst;
            rc = x_inverse(s, bl, EPI_UPDATE, ep, true);
            S.p = s_own;
            t_spec = t_own;
        }
        return rc;
    });
}

}  // namespace mi
