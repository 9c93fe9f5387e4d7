// pystripe's lightsheet correction (pystripe/lightsheet_correct.py correct_lightsheet :31, local_percentile :245, apply_local_function
// :113, as pystripe/core.py:1333-1348 calls it) on batches of equally shaped 2-D tiles.  Every launch covers the whole batch (grid y /
// z = tile).
//
//   row percentile   the lightsheet estimate: windows (1, L) at spacing (1, L), so every window is one run of L samples of one row.
//                    One wave per window: the run is read once into LDS as order-preserving 32-bit keys, every lane ranks up to
//                    four of them per sweep against all L (a broadcast LDS read per comparison; ties broken by position, so ranks
//                    are a permutation) and the two lanes that hold ranks lo and lo + 1 hand their keys over.
//   box percentile   the background estimate (and every other rectangular window): one work-group per centre.  The clipped, stepped
//                    window is staged in LDS once (16-bit keys for integer images, 32-bit for float32) and reduced by a radix
//                    select over a 256-bin LDS histogram, most significant byte first: one pass for uint8, two for uint16, four
//                    for float32.  A thread counts runs of equal bins before it touches the histogram (a smooth background puts
//                    nearly every sample of the first pass into one bin).  The select gives order statistic lo and the number of
//                    samples below and equal to it; statistic lo + 1 is the same value when the equal samples reach past it,
//                    else the smallest larger key (one more sweep).  LDS atomics only.
//   apply            one pass over the image: both order-1 resamplings are evaluated per pixel from the two small grids in float64 in
//                    scipy's order of operations (contraction is off for this whole file), combined with the reference's type
//                    rules, subtracted and stored; optionally the two full-size maps are stored too.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "mi_internal.h"
#include "mi_lightsheet.h"

// numpy and scipy round every product and sum on its own; nothing in this file may be fused
#pragma clang fp contract(off)

namespace mi {
namespace {

using i64 = long long;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// one axis of apply_local_function's sub-grid (:168-198)
struct Axis {
    int extent, selem, spacing, step;
    int n, left;   // centres: left + i * spacing
};

__host__ __device__ inline void axis_window(const Axis& a, int i, int& lo, int& hi) {
    const int c = a.left + i * a.spacing, half = a.selem / 2;
    lo = c - half > 0 ? c - half : 0;
    hi = c + (a.selem - half) < a.extent ? c + (a.selem - half) : a.extent;
}

__host__ __device__ inline int axis_count(const Axis& a, int i) {
    int lo, hi;
    axis_window(a, i, lo, hi);
    return hi > lo ? (hi - lo + a.step - 1) / a.step : 0;
}

Axis make_axis(int extent, int selem, int spacing, int step) {
    Axis a{extent, selem, spacing, step, extent / spacing, 0};
    a.left = a.n ? (extent - (a.n - 1) * spacing) / 2 : 0;
    return a;
}

// numpy.percentile(data, 100 p), method 'linear': q as numpy forms it for integer data (float64) and for float32 data (float32)
struct Pct {
    double q;
    float qf;
};

Pct make_pct(double p) {
    const double hundred_p = 100.0 * p;
    return Pct{hundred_p / 100.0, (float)hundred_p / 100.0f};
}

// indices of the two order statistics among n samples (_get_indexes: at or past the last one, both are the last)
template <bool F32>
__device__ inline void pct_indices(int n, const Pct& p, int& lo, int& hi) {
    int f;
    bool last;
    if (F32) {
        const float v = (float)(n - 1) * p.qf;
        f = (int)floorf(v);
        last = v >= (float)(n - 1);
    } else {
        const double v = (double)(n - 1) * p.q;
        f = (int)floor(v);
        last = v >= (double)(n - 1);
    }
    if (last || f >= n - 1) {
        lo = hi = n - 1;
    } else {
        lo = f < 0 ? 0 : f;
        hi = lo + 1;
    }
}

// _lerp: a + (b - a) g, and b - (b - a) (1 - g) from g = 0.5 on; in the data's float type
template <bool F32>
__device__ inline double pct_value(double a, double b, int n, const Pct& p) {
    if (F32) {
        const float v = (float)(n - 1) * p.qf;
        const float g = v - floorf(v);
        const float af = (float)a, bf = (float)b, d = bf - af;
        if (v >= (float)(n - 1)) return a;
        float r = af + d * g;
        if (g >= 0.5f) r = bf - d * (1.0f - g);
        return (double)r;
    }
    const double v = (double)(n - 1) * p.q;
    const double g = v - floor(v), d = b - a;
    if (v >= (double)(n - 1)) return a;
    double r = a + d * g;
    if (g >= 0.5) r = b - d * (1.0 - g);
    return r;
}

template <class T> struct KeyOf { using type = uint16_t; static constexpr int passes = sizeof(T); static constexpr bool f32 = false; };
template <> struct KeyOf<float> { using type = uint32_t; static constexpr int passes = 4; static constexpr bool f32 = true; };

__device__ inline uint32_t to_key(uint8_t v) { return v; }
__device__ inline uint32_t to_key(uint16_t v) { return v; }
__device__ inline uint32_t to_key(float v) {   // order-preserving: negative floats reversed below the positive ones
    const uint32_t b = __float_as_uint(v);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
template <class T> __device__ inline double from_key(uint32_t k) { return (double)k; }
template <> __device__ inline double from_key<float>(uint32_t k) {
    return (double)__uint_as_float((k & 0x80000000u) ? k ^ 0x80000000u : ~k);
}

// the store into a grid of the map's type: numpy's assignment truncates a float into an integer grid
__device__ inline void store_cell(void* g, int dt, i64 o, double v) {
    if (dt == MI_PS_F32) {
        static_cast<float*>(g)[o] = (float)v;
    } else {
        const double top = dt == MI_PS_U8 ? 255.0 : 65535.0;
        const double c = v > 0.0 ? (v < top ? v : top) : 0.0;   // NaN -> 0
        if (dt == MI_PS_U8) static_cast<uint8_t*>(g)[o] = (uint8_t)c;
        else static_cast<uint16_t*>(g)[o] = (uint16_t)c;
    }
}

__device__ inline double load_cell(const void* g, int dt, i64 o) {
    if (dt == MI_PS_F32) return (double)static_cast<const float*>(g)[o];
    if (dt == MI_PS_U8) return (double)static_cast<const uint8_t*>(g)[o];
    return (double)static_cast<const uint16_t*>(g)[o];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// row percentile: windows (1, L) at spacing (1, L).  Block = 4 waves = 4 windows; LDS: 4 x L keys, then two selected keys per wave.

template <class T>
__global__ void __launch_bounds__(kThreads) row_percentile_kernel(const T* __restrict__ in, i64 tile_px, int nx, int L, int x_first, int cx,
                                                                  i64 nseg, Pct pct, void* grid, int map_dt) {
    extern __shared__ uint32_t lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const i64 seg = (i64)blockIdx.x * kWaves + wave;
    const i64 tile = blockIdx.y;
    const bool active = seg < nseg;
    uint32_t* keys = lds + (size_t)wave * L;
    uint32_t* sel = lds + (size_t)kWaves * L + 2 * wave;
    if (active) {
        const i64 row = seg / cx;
        const int j = (int)(seg - row * cx);
        const T* src = in + tile * tile_px + row * nx + x_first + (i64)j * L;
        for (int i = lane; i < L; i += 64) keys[i] = to_key(src[i]);
    }
    __syncthreads();
    int lo, hi;
    pct_indices<KeyOf<T>::f32>(L, pct, lo, hi);
    if (active) {
        for (int base = 0; base < L; base += 256) {
            uint32_t own[4];
            int idx[4], cnt[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                idx[u] = base + lane + 64 * u;
                own[u] = idx[u] < L ? keys[idx[u]] : 0u;
                cnt[u] = 0;
            }
            for (int j = 0; j < L; ++j) {
                const uint32_t k = keys[j];
#pragma unroll
                for (int u = 0; u < 4; ++u) cnt[u] += (k < own[u] || (k == own[u] && j < idx[u])) ? 1 : 0;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (idx[u] < L && cnt[u] == lo) sel[0] = own[u];
                if (idx[u] < L && cnt[u] == hi) sel[1] = own[u];
            }
        }
    }
    __syncthreads();
    if (active && lane == 0) {
        const double v = pct_value<KeyOf<T>::f32>(from_key<T>(sel[0]), from_key<T>(sel[1]), L, pct);
        store_cell(grid, map_dt, tile * nseg + seg, v);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// box percentile: one work-group per centre, radix select over LDS histograms

template <class T>
__global__ void __launch_bounds__(kThreads) box_percentile_kernel(const T* __restrict__ in, i64 tile_px, int nx, Axis ay, Axis ax, Pct pct, void* grid,
                                                                  int map_dt) {
    using K = typename KeyOf<T>::type;
    constexpr int PASSES = KeyOf<T>::passes;
    extern __shared__ uint32_t lds[];
    K* keys = reinterpret_cast<K*>(lds);
    __shared__ unsigned hist[256];
    __shared__ unsigned wsum[kWaves];
    __shared__ unsigned s_bin, s_below, s_equal, s_min;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int iy = blockIdx.x / ax.n, ix = blockIdx.x - iy * ax.n;
    const i64 tile = blockIdx.y;
    int y0, y1, x0, x1;
    axis_window(ay, iy, y0, y1);
    axis_window(ax, ix, x0, x1);
    const int wy = axis_count(ay, iy), wx = axis_count(ax, ix);
    const int n = wy * wx;   // <= MI_LS_MAX_WINDOW: the host checked every centre
    const i64 cell = tile * ((i64)ay.n * ax.n) + blockIdx.x;
    if (n == 0) {   // an empty window gives 0 (local_percentile :298)
        if (t == 0) store_cell(grid, map_dt, cell, 0.0);
        return;
    }
    const T* src = in + tile * tile_px + (i64)y0 * nx + x0;
    for (int i = t; i < n; i += kThreads) {
        const int ry = i / wx, rx = i - ry * wx;
        keys[i] = (K)to_key(src[(i64)ry * ay.step * nx + rx * ax.step]);
    }
    int lo, hi;
    pct_indices<KeyOf<T>::f32>(n, pct, lo, hi);
    uint32_t prefix = 0;
    unsigned r = (unsigned)lo, equal = 0;
#pragma unroll
    for (int pass = PASSES - 1; pass >= 0; --pass) {
        const int shift = 8 * pass;
        hist[t] = 0;
        if (t == 0) s_min = 0xFFFFFFFFu;
        __syncthreads();   // also orders the staging before the first sweep
        int cur = -1;
        unsigned run = 0;
        for (int i = t; i < n; i += kThreads) {
            const uint32_t k = keys[i];
            if (pass == PASSES - 1 || (k >> (shift + 8)) == prefix) {
                const int b = (k >> shift) & 255;
                if (b != cur) {
                    if (run) atomicAdd(&hist[cur], run);
                    cur = b;
                    run = 0;
                }
                ++run;
            }
        }
        if (run) atomicAdd(&hist[cur], run);
        __syncthreads();
        // inclusive scan of the 256 bins: inside each wave by shuffles, across the four waves through LDS
        const unsigned h = hist[t];
        unsigned incl = h;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned y = __shfl_up(incl, d);
            if (lane >= d) incl += y;
        }
        if (lane == 63) wsum[wave] = incl;
        __syncthreads();
        for (int w = 0; w < wave; ++w) incl += wsum[w];
        if (h && incl - h <= r && r < incl) {   // exactly one bin holds rank r
            s_bin = t;
            s_below = incl - h;
            s_equal = h;
        }
        __syncthreads();
        prefix = (prefix << 8) | s_bin;
        r -= s_below;
        equal = s_equal;
    }
    // prefix is the key of order statistic lo; r of the `equal` samples with that key come before it
    uint32_t next = prefix;
    if (hi != lo && r + 1 >= equal) {   // statistic lo + 1 is the smallest larger key
        uint32_t m = 0xFFFFFFFFu;
        for (int i = t; i < n; i += kThreads) {
            const uint32_t k = keys[i];
            if (k > prefix && k < m) m = k;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint32_t y = __shfl_xor(m, d);
            m = y < m ? y : m;
        }
        if (lane == 0) atomicMin(&s_min, m);
        __syncthreads();
        next = s_min;
    }
    if (t == 0) store_cell(grid, map_dt, cell, pct_value<KeyOf<T>::f32>(from_key<T>(prefix), from_key<T>(next), n, pct));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// scipy.ndimage.zoom(grid, order=1, mode='constant') at one output sample

struct Zoom {
    const void* grid;
    i64 cells;          // per tile
    int ny_in, nx_in;
    double sy, sx;      // (n_in - 1) / (n_out - 1); 1 when n_out == 1
};

__device__ inline double zoom_value(const Zoom& z, int dt, i64 tile, int y, int x) {
    const double cy = (double)y * z.sy, cx = (double)x * z.sx;
    if (cy > (double)(z.ny_in - 1) || cx > (double)(z.nx_in - 1)) return 0.0;   // scipy: past the last node is outside -> cval
    const double fy = floor(cy), fx = floor(cx);
    const double wy0 = 1.0 - (cy - fy), wx0 = 1.0 - (cx - fx);
    const double wy1 = 1.0 - wy0, wx1 = 1.0 - wx0;
    const int iy0 = min((int)fy, z.ny_in - 1), ix0 = min((int)fx, z.nx_in - 1);
    const int iy1 = min(iy0 + 1, z.ny_in - 1), ix1 = min(ix0 + 1, z.nx_in - 1);
    const i64 base = tile * z.cells;
    const double g00 = load_cell(z.grid, dt, base + (i64)iy0 * z.nx_in + ix0), g01 = load_cell(z.grid, dt, base + (i64)iy0 * z.nx_in + ix1);
    const double g10 = load_cell(z.grid, dt, base + (i64)iy1 * z.nx_in + ix0), g11 = load_cell(z.grid, dt, base + (i64)iy1 * z.nx_in + ix1);
    double v = (((g00 * wy0) * wx0 + (g01 * wy0) * wx1) + (g10 * wy1) * wx0) + (g11 * wy1) * wx1;
    if (dt == MI_PS_F32) return (double)(float)v;
    const double top = dt == MI_PS_U8 ? 255.0 : 65535.0;
    v = floor(v + 0.5);
    return v > 0.0 ? (v < top ? v : top) : 0.0;
}

// a value that is already exact in the map's type
__device__ inline void store_exact(void* p, int dt, i64 o, double v) {
    if (dt == MI_PS_F32) static_cast<float*>(p)[o] = (float)v;
    else if (dt == MI_PS_U8) static_cast<uint8_t*>(p)[o] = (uint8_t)v;
    else static_cast<uint16_t*>(p)[o] = (uint16_t)v;
}

__global__ void __launch_bounds__(kThreads) zoom_kernel(Zoom z, int dt, void* out, int ny, int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const i64 tile = blockIdx.z;
    store_exact(out, dt, tile * ((i64)ny * nx) + (i64)y * nx + x, zoom_value(z, dt, tile, y, x));
}

// correct_lightsheet :89-95
struct Combine {
    int img_dt, map_dt;
    int wrap_product;    // bg * k in the map's integer type, modulo its range
    unsigned k;
    double factor;
    float factor_f;
};

__global__ void __launch_bounds__(kThreads) apply_kernel(const void* in, void* out, void* ls_map, void* bg_map, Zoom zl, Zoom zb, Combine c, int ny,
                                                         int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= nx || y >= ny) return;
    const i64 tile = blockIdx.z;
    const i64 o = tile * ((i64)ny * nx) + (i64)y * nx + x;
    const double ls = zoom_value(zl, c.map_dt, tile, y, x), bg = zoom_value(zb, c.map_dt, tile, y, x);
    if (ls_map) store_exact(ls_map, c.map_dt, o, ls);
    if (bg_map) store_exact(bg_map, c.map_dt, o, bg);
    const double v = load_cell(in, c.img_dt, o);
    double prod;
    if (c.wrap_product) prod = (double)(((unsigned)bg * c.k) & (c.map_dt == MI_PS_U8 ? 0xFFu : 0xFFFFu));
    else if (c.map_dt == MI_PS_F32) prod = (double)((float)bg * c.factor_f);
    else prod = bg * c.factor;
    const double m = ls < prod ? ls : prod;
    double take = v < m ? v : m;   // one of the operands, so exact whatever type numpy's minimum promoted to
    if (c.img_dt == MI_PS_F32) {
        static_cast<float*>(out)[o] = (float)v - (float)take;
    } else {
        take = take > 0.0 ? floor(take) : 0.0;   // astype(img.dtype) truncates; take <= v, so the difference stays in range
        store_exact(out, c.img_dt, o, v - take);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// host

size_t dtype_bytes(int dt) { return dt == MI_PS_U8 ? 1 : dt == MI_PS_U16 ? 2 : 4; }
bool dtype_ok(int dt) { return dt == MI_PS_U8 || dt == MI_PS_U16 || dt == MI_PS_F32; }

int check_axis(const char* what, const Axis& a) {
    MI_REQUIRE(a.selem >= 1 && a.spacing >= 1 && a.step >= 1, "mi_lightsheet: %s: selem %d, spacing %d, step %d", what, a.selem, a.spacing, a.step);
    MI_REQUIRE(a.n >= 1, "mi_lightsheet: %s: an extent of %d samples holds no centre at spacing %d", what, a.extent, a.spacing);
    return MI_OK;
}

int axis_most(const Axis& a) {
    int most = 0;
    for (int i = 0; i < a.n; ++i) most = std::max(most, axis_count(a, i));
    return most;
}

bool is_row_grid(const Axis& ay, const Axis& ax) {
    return ay.selem == 1 && ay.spacing == 1 && ay.step == 1 && ax.step == 1 && ax.spacing == ax.selem && ax.selem <= MI_LS_MAX_LENGTH;
}

int check_grid(const Axis& ay, const Axis& ax) {
    MI_TRY(check_axis("axis y", ay));
    MI_TRY(check_axis("axis x", ax));
    if (is_row_grid(ay, ax)) {
        // every window is the full run: left - selem / 2 >= 0 and the last one ends inside the row
        const int first = ax.left - ax.selem / 2;
        MI_REQUIRE(first >= 0 && first + (i64)ax.n * ax.selem <= ax.extent, "mi_lightsheet: row windows leave the image");
        return MI_OK;
    }
    const i64 most = (i64)axis_most(ay) * axis_most(ax);
    if (most > MI_LS_MAX_WINDOW)
        return fail(MI_ERR_UNSUPPORTED, "mi_lightsheet: a window of %lld samples after stepping (at most %d are built)", most, MI_LS_MAX_WINDOW);
    return MI_OK;
}

template <class T>
int launch_grid_t(hipStream_t st, const void* in, int ny, int nx, int cnt, const Axis& ay, const Axis& ax, const Pct& pct, void* grid, int map_dt) {
    const T* src = static_cast<const T*>(in);
    const i64 tile_px = (i64)ny * nx;
    if (is_row_grid(ay, ax)) {
        const int L = ax.selem;
        const i64 nseg = (i64)ny * ax.n;
        const size_t lds = ((size_t)kWaves * L + 2 * kWaves) * sizeof(uint32_t);
        if (lds > 48 * 1024)
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&row_percentile_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(row_percentile_kernel<T>, dim3(cdiv((size_t)nseg, kWaves), cnt), dim3(kThreads), lds, st, src, tile_px, nx, L,
                           ax.left - L / 2, ax.n, nseg, pct, grid, map_dt);
        return launch_check("row_percentile_kernel");
    }
    using K = typename KeyOf<T>::type;
    const size_t lds = ((size_t)axis_most(ay) * axis_most(ax) * sizeof(K) + 15) / 16 * 16;
    if (lds > 48 * 1024)
        MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&box_percentile_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(box_percentile_kernel<T>, dim3((unsigned)(ay.n * ax.n), cnt), dim3(kThreads), lds, st, src, tile_px, nx, ay, ax, pct, grid, map_dt);
    return launch_check("box_percentile_kernel");
}

int launch_grid(hipStream_t st, const void* in, int img_dt, int ny, int nx, int cnt, const Axis& ay, const Axis& ax, const Pct& pct, void* grid,
                int map_dt) {
    if (img_dt == MI_PS_U8) return launch_grid_t<uint8_t>(st, in, ny, nx, cnt, ay, ax, pct, grid, map_dt);
    if (img_dt == MI_PS_U16) return launch_grid_t<uint16_t>(st, in, ny, nx, cnt, ay, ax, pct, grid, map_dt);
    return launch_grid_t<float>(st, in, ny, nx, cnt, ay, ax, pct, grid, map_dt);
}

Zoom make_zoom(const void* grid, const Axis& ay, const Axis& ax, int ny, int nx) {
    Zoom z;
    z.grid = grid;
    z.cells = (i64)ay.n * ax.n;
    z.ny_in = ay.n;
    z.nx_in = ax.n;
    z.sy = ny > 1 ? (double)(ay.n - 1) / (double)(ny - 1) : 1.0;
    z.sx = nx > 1 ? (double)(ax.n - 1) / (double)(nx - 1) : 1.0;
    return z;
}

bool zoom_drops_last(int n_in, int n_out) {
    const double s = n_out > 1 ? (double)(n_in - 1) / (double)(n_out - 1) : 1.0;
    return (double)(n_out - 1) * s > (double)(n_in - 1);
}

constexpr int kMaxChunk = 32768;   // tiles of one launch (grid y / z)

struct Plan {
    int dev = 0, ny = 0, nx = 0, img_dt = 0;
    mi_lightsheet_params prm{};
    mi_lightsheet_info info{};
    Axis ls_y{}, ls_x{}, bg_y{}, bg_x{};
    Pct pct{};
    Combine comb{};
    size_t ls_bytes = 0, bg_bytes = 0;   // per tile, each a multiple of 16
    DevBuf scratch;
    i64 cap = 0;
};

int derive(int ny, int nx, int img_dt, const mi_lightsheet_params& q, Plan& P) {
    MI_REQUIRE(ny > 0 && nx > 0, "mi_lightsheet: tile shape (%d, %d)", ny, nx);
    MI_REQUIRE(dtype_ok(img_dt) && dtype_ok(q.map_dtype), "mi_lightsheet: dtype %d, map dtype %d", img_dt, q.map_dtype);
    MI_REQUIRE(q.percentile >= 0.0 && q.percentile <= 1.0, "mi_lightsheet: percentile %g is outside [0, 1]", q.percentile);
    MI_REQUIRE(q.artifact_length >= 1 && q.background_window_size >= 1, "mi_lightsheet: artifact_length %d, background_window_size %d",
               q.artifact_length, q.background_window_size);
    if (q.artifact_length > MI_LS_MAX_LENGTH)
        return fail(MI_ERR_UNSUPPORTED, "mi_lightsheet: artifact_length %d (at most %d is built)", q.artifact_length, MI_LS_MAX_LENGTH);
    P.ny = ny; P.nx = nx; P.img_dt = img_dt; P.prm = q;
    const int spacing = q.background_spacing > 0 ? q.background_spacing : 25, step = q.background_step > 0 ? q.background_step : 2;
    const int L = q.artifact_length;
    P.ls_y = q.artifact_along_y ? make_axis(ny, L, L, 1) : make_axis(ny, 1, 1, 1);
    P.ls_x = q.artifact_along_y ? make_axis(nx, 1, 1, 1) : make_axis(nx, L, L, 1);
    P.bg_y = make_axis(ny, q.background_window_size, spacing, step);
    P.bg_x = make_axis(nx, q.background_window_size, spacing, step);
    MI_TRY(check_grid(P.ls_y, P.ls_x));
    MI_TRY(check_grid(P.bg_y, P.bg_x));
    P.pct = make_pct(q.percentile);
    const bool img_int = img_dt != MI_PS_F32, map_int = q.map_dtype != MI_PS_F32;
    Combine& c = P.comb;
    c.img_dt = img_dt; c.map_dt = q.map_dtype;
    c.factor = q.lightsheet_vs_background; c.factor_f = (float)q.lightsheet_vs_background;
    c.wrap_product = map_int && (img_int || q.factor_is_integer);
    c.k = 0;
    if (c.wrap_product) {
        const double top = q.map_dtype == MI_PS_U8 ? 255.0 : 65535.0, k = std::trunc(q.lightsheet_vs_background);
        MI_REQUIRE(k >= 0.0 && k <= top, "mi_lightsheet: the integer factor %g does not fit the map's type", k);
        c.k = (unsigned)k;
    }
    mi_lightsheet_info& I = P.info;
    I = mi_lightsheet_info{};
    I.ny = ny; I.nx = nx;
    I.ls_ny = P.ls_y.n; I.ls_nx = P.ls_x.n; I.ls_left_y = P.ls_y.left; I.ls_left_x = P.ls_x.left;
    I.bg_ny = P.bg_y.n; I.bg_nx = P.bg_x.n; I.bg_left_y = P.bg_y.left; I.bg_left_x = P.bg_x.left;
    axis_window(P.bg_y, 0, I.bg_first_y0, I.bg_first_y1);
    axis_window(P.bg_y, P.bg_y.n - 1, I.bg_last_y0, I.bg_last_y1);
    axis_window(P.bg_x, 0, I.bg_first_x0, I.bg_first_x1);
    axis_window(P.bg_x, P.bg_x.n - 1, I.bg_last_x0, I.bg_last_x1);
    I.max_window_samples = std::max(axis_most(P.bg_y) * axis_most(P.bg_x), q.artifact_length);
    I.ls_zero_last_row = zoom_drops_last(P.ls_y.n, ny);
    I.ls_zero_last_col = zoom_drops_last(P.ls_x.n, nx);
    I.bg_zero_last_row = zoom_drops_last(P.bg_y.n, ny);
    I.bg_zero_last_col = zoom_drops_last(P.bg_x.n, nx);
    I.integer_mode = img_int && map_int;
    I.max_batch = std::min(q.max_batch > 0 ? q.max_batch : 16, kMaxChunk);
    const size_t mb = dtype_bytes(q.map_dtype);
    P.ls_bytes = ((size_t)I.ls_ny * I.ls_nx * mb + 15) / 16 * 16;
    P.bg_bytes = ((size_t)I.bg_ny * I.bg_nx * mb + 15) / 16 * 16;
    I.scratch_bytes_per_tile = P.ls_bytes + P.bg_bytes;
    return MI_OK;
}

int run_chunk(Plan& P, hipStream_t st, const void* in, void* out, void* ls_map, void* bg_map, int cnt) {
    // grids of the chunk: [tile][cells] of the lightsheet estimate, then of the background
    char* ls_grid = P.scratch.as<char>();
    char* bg_grid = ls_grid + P.ls_bytes * (size_t)P.cap;
    MI_TRY(launch_grid(st, in, P.img_dt, P.ny, P.nx, cnt, P.ls_y, P.ls_x, P.pct, ls_grid, P.prm.map_dtype));
    MI_TRY(launch_grid(st, in, P.img_dt, P.ny, P.nx, cnt, P.bg_y, P.bg_x, P.pct, bg_grid, P.prm.map_dtype));
    const Zoom zl = make_zoom(ls_grid, P.ls_y, P.ls_x, P.ny, P.nx), zb = make_zoom(bg_grid, P.bg_y, P.bg_x, P.ny, P.nx);
    hipLaunchKernelGGL(apply_kernel, dim3(cdiv(P.nx, 64), cdiv(P.ny, 4), cnt), dim3(kThreads), 0, st, in, out, ls_map, bg_map, zl, zb, P.comb, P.ny,
                       P.nx);
    return launch_check("apply_kernel");
}

}  // namespace
}  // namespace mi

using mi::Plan;

extern "C" int mi_lightsheet_derive(int ny, int nx, int img_dtype, const mi_lightsheet_params* params, mi_lightsheet_info* info) {
    MI_REQUIRE(params && info, "mi_lightsheet_derive: null pointer");
    Plan P;
    MI_TRY(mi::derive(ny, nx, img_dtype, *params, P));
    *info = P.info;
    return MI_OK;
}

extern "C" int mi_lightsheet_plan_create(int dev, int ny, int nx, int img_dtype, const mi_lightsheet_params* params, void** plan) {
    MI_REQUIRE(params && plan, "mi_lightsheet_plan_create: null pointer");
    *plan = nullptr;
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    const int rc = mi::derive(ny, nx, img_dtype, *params, *P);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    *plan = P;
    return MI_OK;
}

extern "C" int mi_lightsheet_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_lightsheet_plan_info(void* plan, mi_lightsheet_info* info) {
    MI_REQUIRE(plan && info, "mi_lightsheet_plan_info: null pointer");
    *info = static_cast<Plan*>(plan)->info;
    return MI_OK;
}

extern "C" int mi_lightsheet_run(void* plan, void* stream, const void* in, void* out, void* ls_map, void* bg_map, int64_t count) {
    MI_REQUIRE(plan && in && out, "mi_lightsheet_run: null pointer");
    MI_REQUIRE(count >= 0, "mi_lightsheet_run: count %lld", (long long)count);
    Plan& P = *static_cast<Plan*>(plan);
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    const int64_t want = std::min<int64_t>(count, P.info.max_batch);
    if (want > P.cap) {
        MI_HIP(hipStreamSynchronize(st));   // work of an earlier call may still use the smaller scratch
        P.cap = 0;
        MI_TRY(P.scratch.alloc(P.info.scratch_bytes_per_tile * (size_t)want));
        P.cap = want;
    }
    const size_t img_bytes = (size_t)P.ny * P.nx * mi::dtype_bytes(P.img_dt), map_bytes = (size_t)P.ny * P.nx * mi::dtype_bytes(P.prm.map_dtype);
    for (int64_t t0 = 0; t0 < count; t0 += P.cap) {
        const int cnt = (int)std::min<int64_t>(P.cap, count - t0);
        MI_TRY(mi::run_chunk(P, st, static_cast<const char*>(in) + (size_t)t0 * img_bytes, static_cast<char*>(out) + (size_t)t0 * img_bytes,
                             ls_map ? static_cast<char*>(ls_map) + (size_t)t0 * map_bytes : nullptr,
                             bg_map ? static_cast<char*>(bg_map) + (size_t)t0 * map_bytes : nullptr, cnt));
    }
    return MI_OK;
}

extern "C" int mi_lightsheet_local_percentile(int dev, void* stream, const void* in, int img_dtype, int ny, int nx, int64_t count, int selem_y,
                                              int selem_x, int spacing_y, int spacing_x, int step_y, int step_x, double percentile,
                                              int interpolate, void* out, int out_dtype) {
    MI_REQUIRE(in && out, "mi_lightsheet_local_percentile: null pointer");
    MI_REQUIRE(ny > 0 && nx > 0 && count >= 0, "mi_lightsheet_local_percentile: shape (%d, %d), count %lld", ny, nx, (long long)count);
    MI_REQUIRE(mi::dtype_ok(img_dtype) && mi::dtype_ok(out_dtype), "mi_lightsheet_local_percentile: dtype %d -> %d", img_dtype, out_dtype);
    MI_REQUIRE(percentile >= 0.0 && percentile <= 1.0, "mi_lightsheet_local_percentile: percentile %g is outside [0, 1]", percentile);
    MI_REQUIRE(interpolate == 0 || interpolate == 1, "mi_lightsheet_local_percentile: interpolate %d (0 or 1)", interpolate);
    MI_REQUIRE(selem_y >= 1 && selem_x >= 1 && spacing_y >= 1 && spacing_x >= 1 && step_y >= 1 && step_x >= 1,
               "mi_lightsheet_local_percentile: selem, spacing and step must be positive");
    const mi::Axis ay = mi::make_axis(ny, selem_y, spacing_y, step_y), ax = mi::make_axis(nx, selem_x, spacing_x, step_x);
    MI_TRY(mi::check_grid(ay, ax));
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(dev));
    hipStream_t st = mi::as_stream(stream);
    const mi::Pct pct = mi::make_pct(percentile);
    const size_t cell_bytes = (size_t)ay.n * ax.n * mi::dtype_bytes(out_dtype);
    const size_t img_bytes = (size_t)ny * nx * mi::dtype_bytes(img_dtype), map_bytes = (size_t)ny * nx * mi::dtype_bytes(out_dtype);
    const int64_t chunk = std::min<int64_t>(count, interpolate ? 64 : mi::kMaxChunk);
    mi::DevBuf grids;
    if (interpolate) MI_TRY(grids.alloc(cell_bytes * (size_t)chunk));
    for (int64_t t0 = 0; t0 < count; t0 += chunk) {
        const int cnt = (int)std::min<int64_t>(chunk, count - t0);
        const char* src = static_cast<const char*>(in) + (size_t)t0 * img_bytes;
        if (!interpolate) {
            MI_TRY(mi::launch_grid(st, src, img_dtype, ny, nx, cnt, ay, ax, pct, static_cast<char*>(out) + (size_t)t0 * cell_bytes, out_dtype));
            continue;
        }
        MI_TRY(mi::launch_grid(st, src, img_dtype, ny, nx, cnt, ay, ax, pct, grids.p, out_dtype));
        const mi::Zoom z = mi::make_zoom(grids.p, ay, ax, ny, nx);
        hipLaunchKernelGGL(mi::zoom_kernel, dim3(mi::cdiv(nx, 64), mi::cdiv(ny, 4), cnt), dim3(mi::kThreads), 0, st, z, out_dtype,
                           static_cast<char*>(out) + (size_t)t0 * map_bytes, ny, nx);
        MI_TRY(mi::launch_check("zoom_kernel"));
    }
    MI_HIP(hipStreamSynchronize(st));   // the grids go back to the pool
    return MI_OK;
}
