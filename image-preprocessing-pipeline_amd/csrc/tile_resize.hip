// process_img's resize of a tile to new_size (pystripe/core.py:1356-1359) on batches of equally shaped 2-D tiles, as DESIGN.md
// section 14 restates skimage.transform.resize without a pre-filter: scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) and a
// clip to the tile's own [min, max].  Three launches per chunk of tiles, all on the caller's stream:
//
//   init      the per-tile (min, max) keys of the chunk to (all ones, 0).
//   min / max one pass over the input.  A tile is a run of tile_px samples whose start need not be 16-byte aligned: the samples before
//             the first aligned address and behind the last whole vector are read one by one by the tile's first work-group, the
//             body as 16-byte vectors (grid-stride).  Samples become order-preserving 32-bit keys (the value for integers, the
//             sign-folded bit pattern for float32), are reduced over the wave with shuffles, over the work-group through LDS, and
//             the work-group's pair goes to the tile's slot with one integer atomic min and max (exact in any order).  Every tile has
//             a 128-byte line of its own and at most 2048 / tiles work-groups (16 .. 256): with 256 work-groups for each of 16
//             tiles and all slots on one line the 8192 atomics took 91 us, one after the other, where the pass itself takes 26.
//   zoom      grid (x blocks, row groups, tile).  A thread owns kXpt output columns, kThreads apart, so that the lanes of a wave own
//             64 adjacent columns: a gather of theirs touches one or two cache lines of a source row and a store is one run of 64
//             samples (with four ADJACENT columns per thread a gather spread over four lines and the kernel took 241 us instead
//             of 131).  The columns' table entries (i0, i1, t) are read once and kept for the kRows output rows of the work-group;
//             per row the two source rows y0, y1 and the weight are the same for the whole work-group (they depend on blockIdx
//             alone).  Recipe, float64, every product and sum rounded on its own:
//                 s = (a[y0][x0] wy0) wx0 + (a[y0][x1] wy0) wx1 + (a[y1][x0] wy1) wx0 + (a[y1][x1] wy1) wx1,  left to right,
//             then float32: (float)s clipped to [min, max]; integers: s clipped, truncated, in the store.
// The tables are made on the host in float64 (mi_tile_resize_tables, the same function the tests read) and live in the plan.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "mi_internal.h"
#include "mi_pystripe.h"
#include "mi_tile_resize.h"

// scipy rounds every product and sum on its own; nothing in this file may be fused
#pragma clang fp contract(off)

namespace mi {
namespace {

using i64 = long long;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kXpt = 4;    // output columns of one thread, kThreads apart
constexpr int kRows = 8;   // output rows of one work-group
constexpr int kMaxChunk = 32768;   // tiles of one launch (grid y / z)
constexpr int kSlot = 32;          // 32-bit words between the (min, max) pairs of two tiles: one 128-byte line per tile

size_t dtype_bytes(int dt) { return dt == MI_PS_U8 ? 1 : dt == MI_PS_U16 ? 2 : 4; }
bool dtype_ok(int dt) { return dt == MI_PS_U8 || dt == MI_PS_U16 || dt == MI_PS_F32; }

// order-preserving 32-bit keys
__device__ inline uint32_t to_key(uint8_t v) { return v; }
__device__ inline uint32_t to_key(uint16_t v) { return v; }
__device__ inline uint32_t to_key(float v) {
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
template <class T> __device__ inline T from_key(uint32_t k) { return (T)k; }
template <> __device__ inline float from_key<float>(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__global__ void __launch_bounds__(kThreads) minmax_init_kernel(uint32_t* mm, int cnt) {
    const int t = blockIdx.x * kThreads + threadIdx.x;
    if (t < cnt) {
        mm[kSlot * t] = 0xffffffffu;
        mm[kSlot * t + 1] = 0u;
    }
}

template <class T>
__global__ void __launch_bounds__(kThreads) minmax_kernel(const T* __restrict__ in, i64 tile_px, uint32_t* __restrict__ mm) {
    constexpr int kVe = 16 / (int)sizeof(T);
    const T* a = in + (i64)blockIdx.y * tile_px;
    i64 head = (i64)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(a) & 15u)) & 15u) / sizeof(T));
    if (head > tile_px) head = tile_px;
    const i64 nvec = (tile_px - head) / kVe, tail = head + nvec * kVe;
    uint32_t lo = 0xffffffffu, hi = 0u;
    const uint4* body = reinterpret_cast<const uint4*>(a + head);
#pragma unroll 4
    for (i64 v = (i64)blockIdx.x * kThreads + threadIdx.x; v < nvec; v += (i64)gridDim.x * kThreads) {
        const uint4 q = body[v];
        T e[kVe];
        memcpy(e, &q, 16);
#pragma unroll
        for (int j = 0; j < kVe; ++j) {
            const uint32_t k = to_key(e[j]);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
    if (blockIdx.x == 0) {   // fewer than 2 kVe samples: [0, head) and [tail, tile_px)
        const i64 rest = head + (tile_px - tail);
        for (i64 r = threadIdx.x; r < rest; r += kThreads) {
            const uint32_t k = to_key(a[r < head ? r : tail + (r - head)]);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const uint32_t l2 = (uint32_t)__shfl_xor((int)lo, s), h2 = (uint32_t)__shfl_xor((int)hi, s);
        lo = l2 < lo ? l2 : lo;
        hi = h2 > hi ? h2 : hi;
    }
    __shared__ uint32_t part[2 * kWaves];
    if ((threadIdx.x & 63) == 0) {
        part[2 * (threadIdx.x >> 6)] = lo;
        part[2 * (threadIdx.x >> 6) + 1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kWaves; ++w) {
            lo = part[2 * w] < lo ? part[2 * w] : lo;
            hi = part[2 * w + 1] > hi ? part[2 * w + 1] : hi;
        }
        atomicMin(&mm[kSlot * blockIdx.y], lo);
        atomicMax(&mm[kSlot * blockIdx.y + 1], hi);
    }
}

struct Geom {
    int ny, nx, my, mx;
};

struct Tables {   // device pointers, one entry per output row / column
    const int *yi0, *yi1, *xi0, *xi1;
    const double *yt, *xt;
};

template <class T> __device__ inline T finish(double s, T lo, T hi) {   // integer tile: the float64 clipped, then truncated
    const double l = (double)lo, h = (double)hi;
    s = s < l ? l : s;
    s = s > h ? h : s;
    return (T)s;
}
template <> __device__ inline float finish<float>(double s, float lo, float hi) {   // float32 tile: rounded, then clipped
    float f = (float)s;
    f = f < lo ? lo : f;
    return f > hi ? hi : f;
}

template <class T>
__global__ void __launch_bounds__(kThreads) zoom_kernel(const T* __restrict__ in, T* __restrict__ out, Geom g, Tables tb,
                                                        const uint32_t* __restrict__ mm) {
    const int x_first = blockIdx.x * kThreads * kXpt + threadIdx.x;   // column j of the thread: x_first + j kThreads
    if (x_first >= g.mx) return;   // no barrier below
    const int tile = blockIdx.z;
    const T* src = in + (i64)tile * g.ny * g.nx;
    T* dst = out + (i64)tile * g.my * g.mx;
    const T lo = from_key<T>(mm[kSlot * tile]), hi = from_key<T>(mm[kSlot * tile + 1]);
    int x0[kXpt], x1[kXpt];
    double wx0[kXpt], wx1[kXpt];
#pragma unroll
    for (int j = 0; j < kXpt; ++j) {
        const int x = x_first + j * kThreads < g.mx ? x_first + j * kThreads : x_first;   // a dead column repeats the first: in bounds, never stored
        x0[j] = tb.xi0[x];
        x1[j] = tb.xi1[x];
        wx1[j] = tb.xt[x];
        wx0[j] = 1.0 - wx1[j];
    }
    const int y_first = blockIdx.y * kRows;
    for (int r = 0; r < kRows; ++r) {
        const int y = y_first + r;
        if (y >= g.my) break;
        const T* row0 = src + (i64)tb.yi0[y] * g.nx;
        const T* row1 = src + (i64)tb.yi1[y] * g.nx;
        const double wy1 = tb.yt[y], wy0 = 1.0 - wy1;
        T res[kXpt];
#pragma unroll
        for (int j = 0; j < kXpt; ++j) {
            double s = ((double)row0[x0[j]] * wy0) * wx0[j];
            s = s + ((double)row0[x1[j]] * wy0) * wx1[j];
            s = s + ((double)row1[x0[j]] * wy1) * wx0[j];
            s = s + ((double)row1[x1[j]] * wy1) * wx1[j];
            res[j] = finish<T>(s, lo, hi);
        }
        T* o = dst + (i64)y * g.mx + x_first;
#pragma unroll
        for (int j = 0; j < kXpt; ++j)
            if (x_first + j * kThreads < g.mx) o[j * kThreads] = res[j];
    }
}

// one axis of the recipe, n samples -> m samples; the indices are kept inside [0, n - 1] whatever the arithmetic gives
void axis_tables(int n, int m, int* i0, int* i1, double* t) {
    const double z = (double)n / (double)m, last = (double)(n - 1);
    for (int k = 0; k < m; ++k) {
        double c = ((double)k + 0.5) * z - 0.5;
        if (n == 1) c = 0.0;
        else if (c < 0.0) c = -c;
        else if (c > last) c = 2.0 * last - c;
        const double f = std::floor(c);
        int a = (int)f, b = a + 1;
        if (b > n - 1) b = n > 1 ? 2 * (n - 1) - b : 0;
        i0[k] = std::min(std::max(a, 0), n - 1);
        i1[k] = std::min(std::max(b, 0), n - 1);
        t[k] = c - f;
    }
}

struct Plan {
    int dev = 0, dt = 0, max_batch = 0;
    Geom g{};
    Tables tb{};
    DevBuf tables, minmax;   // the six tables back to back; (min, max) keys of max_batch tiles, kSlot words apart
};

int check_shape(const char* who, int ny, int nx, int my, int mx) {
    MI_REQUIRE(ny >= 1, "%s: ny=%d: an extent of 1 or more is expected", who, ny);
    MI_REQUIRE(nx >= 1, "%s: nx=%d: an extent of 1 or more is expected", who, nx);
    MI_REQUIRE(my >= 1, "%s: my=%d: an extent of 1 or more is expected", who, my);
    MI_REQUIRE(mx >= 1, "%s: mx=%d: an extent of 1 or more is expected", who, mx);
    return MI_OK;
}

template <class T>
int run_chunk_t(const Plan& P, hipStream_t st, const void* in, void* out, int cnt) {
    const Geom& g = P.g;
    uint32_t* mm = P.minmax.as<uint32_t>();
    const i64 tile_px = (i64)g.ny * g.nx;
    hipLaunchKernelGGL(minmax_init_kernel, dim3(cdiv((size_t)cnt, kThreads)), dim3(kThreads), 0, st, mm, cnt);
    MI_TRY(launch_check("tile_resize minmax_init_kernel"));
    const size_t vecs = (size_t)tile_px / (16 / sizeof(T));
    // atomics on one line retire one after the other (about 90 per microsecond): few work-groups per tile when the tiles fill the device
    const unsigned most = (unsigned)std::min(std::max(2048 / cnt, 16), 256);
    const unsigned blocks = std::min(std::max(cdiv(vecs, (size_t)kThreads * 4), 1u), most);
    hipLaunchKernelGGL(minmax_kernel<T>, dim3(blocks, cnt), dim3(kThreads), 0, st, static_cast<const T*>(in), tile_px, mm);
    MI_TRY(launch_check("tile_resize minmax_kernel"));
    hipLaunchKernelGGL(zoom_kernel<T>, dim3(cdiv((size_t)g.mx, (size_t)kThreads * kXpt), cdiv((size_t)g.my, kRows), cnt), dim3(kThreads), 0, st,
                       static_cast<const T*>(in), static_cast<T*>(out), g, P.tb, mm);
    return launch_check("tile_resize zoom_kernel");
}

}  // namespace
}  // namespace mi

using mi::Plan;

extern "C" int mi_tile_resize_tables(int n, int m, int* i0, int* i1, double* t) {
    MI_REQUIRE(i0 && i1 && t, "mi_tile_resize_tables: null pointer");
    MI_REQUIRE(n >= 1, "mi_tile_resize_tables: n=%d: an extent of 1 or more is expected", n);
    MI_REQUIRE(m >= 1, "mi_tile_resize_tables: m=%d: an extent of 1 or more is expected", m);
    mi::axis_tables(n, m, i0, i1, t);
    return MI_OK;
}

extern "C" int mi_tile_resize_plan_create(int dev, int ny, int nx, int my, int mx, int dtype, int max_batch, void** plan) {
    MI_REQUIRE(plan, "mi_tile_resize_plan_create: null pointer");
    *plan = nullptr;
    MI_TRY(mi::check_shape("mi_tile_resize_plan_create", ny, nx, my, mx));
    MI_REQUIRE(mi::dtype_ok(dtype), "mi_tile_resize_plan_create: dtype=%d: MI_PS_U8, MI_PS_U16 or MI_PS_F32 is expected", dtype);
    MI_REQUIRE((long long)ny * nx <= INT32_MAX && (long long)my * mx <= INT32_MAX,
               "mi_tile_resize_plan_create: a tile of (%d, %d) -> (%d, %d): at most 2^31 - 1 samples per tile", ny, nx, my, mx);
    MI_REQUIRE(mx <= (1 << 30), "mi_tile_resize_plan_create: mx=%d: at most 2^30 output columns are built", mx);
    MI_REQUIRE(my <= 65535 * mi::kRows, "mi_tile_resize_plan_create: my=%d: at most %d output rows are built", my, 65535 * mi::kRows);
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    P->dt = dtype;
    P->g = mi::Geom{ny, nx, my, mx};
    P->max_batch = std::min(max_batch > 0 ? max_batch : 16, mi::kMaxChunk);
    // [yi0 | yi1 | xi0 | xi1] as int, then [yt | xt] as double on an 8-byte boundary
    const size_t ints = 2 * ((size_t)my + mx), int_bytes = (ints * sizeof(int) + 15) / 16 * 16, bytes = int_bytes + ((size_t)my + mx) * sizeof(double);
    std::vector<char> host(bytes, 0);
    int* hi = reinterpret_cast<int*>(host.data());
    double* hd = reinterpret_cast<double*>(host.data() + int_bytes);
    mi::axis_tables(ny, my, hi, hi + my, hd);
    mi::axis_tables(nx, mx, hi + 2 * (size_t)my, hi + 2 * (size_t)my + mx, hd + my);
    int rc = P->tables.alloc(bytes);
    if (rc == MI_OK) rc = P->minmax.alloc((size_t)P->max_batch * mi::kSlot * sizeof(uint32_t));
    if (rc == MI_OK && hipMemcpy(P->tables.p, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess)
        rc = mi::fail(MI_ERR_HIP, "mi_tile_resize_plan_create: the upload of the tables failed");
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    const int* di = P->tables.as<int>();
    const double* dd = reinterpret_cast<const double*>(P->tables.as<char>() + int_bytes);
    P->tb = mi::Tables{di, di + my, di + 2 * (size_t)my, di + 2 * (size_t)my + mx, dd, dd + my};
    *plan = P;
    return MI_OK;
}

extern "C" int mi_tile_resize_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_tile_resize_run(void* plan, void* stream, const void* in, void* out, int64_t count) {
    MI_REQUIRE(plan && in && out, "mi_tile_resize_run: null pointer");
    MI_REQUIRE(count >= 0, "mi_tile_resize_run: count=%lld", (long long)count);
    const Plan& P = *static_cast<Plan*>(plan);
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    const mi::Geom& g = P.g;
    const size_t sb = mi::dtype_bytes(P.dt);
    MI_REQUIRE(reinterpret_cast<uintptr_t>(in) % sb == 0 && reinterpret_cast<uintptr_t>(out) % sb == 0, "mi_tile_resize_run: in / out are not aligned to a sample");
    const size_t in_bytes = (size_t)g.ny * g.nx * sb, out_bytes = (size_t)g.my * g.mx * sb;
    if (g.ny == g.my && g.nx == g.mx) {   // equal shapes: the copy (every weight would be 1 or 0)
        MI_HIP(hipMemcpyAsync(out, in, in_bytes * (size_t)count, hipMemcpyDeviceToDevice, st));
        return MI_OK;
    }
    for (int64_t t0 = 0; t0 < count; t0 += P.max_batch) {
        const int cnt = (int)std::min<int64_t>(P.max_batch, count - t0);
        const void* src = static_cast<const char*>(in) + (size_t)t0 * in_bytes;
        void* dst = static_cast<char*>(out) + (size_t)t0 * out_bytes;
        if (P.dt == MI_PS_U8) MI_TRY(mi::run_chunk_t<uint8_t>(P, st, src, dst, cnt));
        else if (P.dt == MI_PS_U16) MI_TRY(mi::run_chunk_t<uint16_t>(P, st, src, dst, cnt));
        else MI_TRY(mi::run_chunk_t<float>(P, st, src, dst, cnt));
    }
    return MI_OK;
}
