// pystripe's automatic clips (pystripe_internal.h: clips): range, histogram and triple per tile around the search of thresholds.hip.
#include <algorithm>
#include <cmath>

#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

// filter_streaks :1066-1077: threshold_multiotsu(log1p(tile), classes=4).  The value of a sample of the log image: for an
// integer-kind tile table[code] (numpy's float32 log1p of the code, so that the counts are numpy.histogram's exactly; the staged
// float of a max / min down-sample is a whole code), else log1pf on load (s.logp).
__device__ __forceinline__ float auto_value(const Src& s, const float* table, int ncodes, i64 tile, int y, int x) {
    const float v = src_load(s, tile, y, x);
    return table ? table[min(max((int)v, 0), ncodes - 1)] : v;
}

// finite range per tile as keys (thresholds.hip's minmax_kernel on this source); rows over the work-groups of grid.x
__global__ void __launch_bounds__(256) auto_range_kernel(Src s, const float* table, int ncodes, unsigned* keys, int* nonfinite) {
    const i64 tile = blockIdx.y;
    float lo = INFINITY, hi = -INFINITY;
    int bad = 0;
    for (int y = blockIdx.x; y < s.ny; y += gridDim.x)
        for (int x = threadIdx.x; x < s.nx; x += 256) {
            const float v = auto_value(s, table, ncodes, tile, y, x);
            if (fabsf(v) < INFINITY) {
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
            } else {
                bad = 1;
            }
        }
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
        bad |= __shfl_xor(bad, d);
    }
    // one pair of atomics per work-group: every group of a tile lands on the same two addresses, and they run one after the other
    __shared__ float wlo[4], whi[4];
    __shared__ int wbad[4];
    if ((threadIdx.x & 63u) == 0) {
        wlo[threadIdx.x >> 6] = lo;
        whi[threadIdx.x >> 6] = hi;
        wbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) {
            lo = fminf(lo, wlo[w]);
            hi = fmaxf(hi, whi[w]);
            bad |= wbad[w];
        }
        if (lo <= hi) {
            atomicMin(&keys[2 * tile], histdev::float_key(lo));
            atomicMax(&keys[2 * tile + 1], histdev::float_key(hi));
        }
        if (bad) atomicOr(&nonfinite[tile], 1);
    }
}

// numpy.histogram(., 256) per tile (thresholds.hip's hist256_kernel on this source)
__global__ void __launch_bounds__(256) auto_hist_kernel(Src s, const float* table, int ncodes, const float* edges, const int* nonfinite,
                                                        unsigned long long* counts) {
    __shared__ float e[MI_HIST_BINS + 1];
    __shared__ unsigned h[4][MI_HIST_BINS];
    const i64 tile = blockIdx.y;
    const int t = threadIdx.x;
    if (nonfinite[tile]) return;   // the whole work-group
    e[t] = edges[tile * (MI_HIST_BINS + 1) + t];
    if (t == 0) e[MI_HIST_BINS] = edges[tile * (MI_HIST_BINS + 1) + MI_HIST_BINS];
    for (int w = 0; w < 4; ++w) h[w][t] = 0;
    __syncthreads();
    const float e0 = e[0];
    const float scale = 256.0f / (e[MI_HIST_BINS] - e0);
    unsigned* mine = h[t >> 6];
    for (int y = blockIdx.x; y < s.ny; y += gridDim.x)
        for (int x = t; x < s.nx; x += 256) histdev::wave_count(mine, histdev::hist_bin(e, e0, scale, auto_value(s, table, ncodes, tile, y, x)));
    __syncthreads();
    unsigned sum = 0;
    for (int w = 0; w < 4; ++w) sum += h[w][t];
    if (sum) atomicAdd(&counts[tile * MI_HIST_BINS + t], (unsigned long long)sum);
}

// The triple and the status of every tile: given clips keep their slot, an estimated one is the float32 centre of the bin the search
// named; min is raised to log1p(1); the asserts of correct_bleaching :524-528 on the result.  A tile without usable clips is zeroed
// through `varies`; its estimated slots hold NaN unless the order check failed (the triple is then what the caller reports).
// padc (constant padding with an estimated minimum, else null): log1p of the minimum BEFORE it is raised, per tile at stride
// padc_ts -- filter_streaks :1101-1105 pads with log1p of the threshold itself; 0 for a tile without usable clips (it is zeroed).
__global__ void __launch_bounds__(64) auto_clips_kernel(int cnt, int bits, float gmin, float gmed, float gmax, double floor_lo, const float* edges,
                                                        const int* indices, const int* otsu_status, const int* nonfinite, int uniform_rule,
                                                        int* varies, float* clips, int* status, float* padc, i64 padc_ts) {
    const int tile = blockIdx.x * 64 + threadIdx.x;
    if (tile >= cnt) return;
    float c[3] = {gmin, gmed, gmax};
    int st = MI_PS_CLIPS_OK;
    if (uniform_rule && !varies[tile]) st = MI_PS_CLIPS_UNIFORM;
    else if (nonfinite[tile]) st = MI_PS_CLIPS_NONFINITE;
    else if (otsu_status[tile] == MI_OTSU_TOO_FEW_VALUES) st = MI_PS_CLIPS_TOO_FEW;
    const float* e = edges + (i64)tile * (MI_HIST_BINS + 1);
    for (int k = 0; k < 3; ++k)
        if ((bits >> k) & 1) {
            const int i = min(max(indices[tile * (MI_OTSU_MAX_CLASSES - 1) + k], 0), MI_HIST_BINS - 1);
            c[k] = st == MI_PS_CLIPS_OK ? (e[i] + e[i + 1]) / 2.0f : NAN;
        }
    if (st == MI_PS_CLIPS_OK && !(c[0] >= 0.f && c[1] > c[0] && c[2] > c[0] && c[2] > c[1])) st = MI_PS_CLIPS_ORDER;
    if (padc) padc[tile * padc_ts] = st == MI_PS_CLIPS_OK ? (float)log1p((double)c[0]) : 0.f;
    if (st == MI_PS_CLIPS_OK) c[0] = (float)fmax((double)c[0], floor_lo);
    if (st > 0) varies[tile] = 0;
    clips[3 * tile] = c[0]; clips[3 * tile + 1] = c[1]; clips[3 * tile + 2] = c[2];
    status[tile] = st;
}

}  // namespace

int upload_log_table(Plan& P, const float* table) {
    if (!P.ncodes) return MI_OK;
    std::vector<float> own;
    if (!table) {
        own.resize((size_t)P.ncodes);
        for (int c = 0; c < P.ncodes; ++c) own[(size_t)c] = log1pf((float)c);
        table = own.data();
    }
    if (!P.table_buf.p) MI_TRY(P.table_buf.alloc(sizeof(float) * (size_t)P.ncodes));
    MI_HIP(hipMemcpy(P.table_buf.p, table, sizeof(float) * (size_t)P.ncodes, hipMemcpyHostToDevice));
    return MI_OK;
}

// range, edges, histogram, search, triple.  Everything stays on the stream.
int run_auto_clips(const Plan& P, hipStream_t st, Src src, int cnt, int* varies, float* clips, int* status) {
    const mi_pystripe_info& I = P.info;
    const mi_pystripe_params& q = P.prm;
    char* base = P.auto_buf.as<char>();
    const size_t cap = (size_t)P.cap;
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(base);
    unsigned long long* work = counts + MI_HIST_BINS * cap;
    float* edges = reinterpret_cast<float*>(work + cap);
    unsigned* keys = reinterpret_cast<unsigned*>(edges + (MI_HIST_BINS + 1) * cap);
    int* indices = reinterpret_cast<int*>(keys + 2 * cap);
    int* nonfinite = indices + (MI_OTSU_MAX_CLASSES - 1) * cap;
    int* nvalues = nonfinite + cap;
    int* otsu_status = nvalues + cap;
    const float* table = nullptr;
    if (I.integer_kind) table = P.table_buf.as<float>();
    else src.logp = 1;
    MI_TRY(hist_init_launch(st, keys, nonfinite, counts, cnt));
    const dim3 grid((unsigned)std::min(I.ny, 256), cnt);   // rows over the groups of a tile: few groups, few same-address atomics at the end
    hipLaunchKernelGGL(auto_range_kernel, grid, dim3(256), 0, st, src, table, P.ncodes, keys, nonfinite);
    MI_TRY(launch_check("auto_range_kernel"));
    MI_TRY(hist_edges_launch(st, keys, edges, cnt));
    hipLaunchKernelGGL(auto_hist_kernel, grid, dim3(256), 0, st, src, table, P.ncodes, edges, nonfinite, counts);
    MI_TRY(launch_check("auto_hist_kernel"));
    MI_TRY(multiotsu_launch(st, counts, cnt, MI_OTSU_MAX_CLASSES, indices, nvalues, otsu_status, work));
    float* padc = P.valpad && q.padding_mode == MI_PS_CONSTANT && (P.au & MI_PS_AUTO_MIN) ? P.buf(P.off_pvec) : nullptr;
    hipLaunchKernelGGL(auto_clips_kernel, dim3(cdiv((size_t)cnt, 64)), dim3(64), 0, st, cnt, P.au, (float)q.bleach_clip_min,
                       (float)q.bleach_clip_med, (float)q.bleach_clip_max, std::log1p(1.0), edges, indices, otsu_status, nonfinite,
                       !q.keep_uniform && !q.log_output, varies, clips, status, padc, (i64)P.sz_pvec);
    return launch_check("auto_clips_kernel");
}

}  // namespace ps
}  // namespace mi
