// The isotropic down-sampled volume of the per-slice pass (parallel_image_processor.py :156-187, :371-384, :411-435, :722; the
// definition is in include/mi_isodown.h and DESIGN section 14).
//
//   halve      the whole chain of max / mean halvings of a slice in one kernel.  A work-group owns a tile of the halved plane and
//              the (tile << ky) x (tile << kx) source block behind it.  A lane reads 16 bytes of one row (of two rows when the chain
//              starts with a y halving), converts to float32 and applies the leading y step and the x steps that follow it on its
//              registers; the rest of the chain runs in LDS, ping-pong between two buffers.  Samples past the slice are loaded as
//              zeros: every level's zero pad behind an odd extent then is where block_reduce puts it, because a sample past a
//              level's extent is made of samples past the extent of the level below.  Every lane compares what it loaded with
//              sample (0, 0); a difference is recorded by a plain store of 1 into the slice's flag word.
//   resize     per-axis Gaussian taps (double accumulation, float32 store between the axes, mirror indexing of any reach), the
//              order-1 interpolation of all axes in one kernel (double), the clip to the input's min / max (a two-stage reduction).
//   reduce z   max / mean rounds over the planes of a group, one lane per pixel, in place.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mi_internal.h"
#include "mi_isodown.h"

// numpy rounds every sum and product on its own
#pragma clang fp contract(off)

namespace mi {
namespace {

using i64 = long long;
constexpr int kThreads = 256;
constexpr int kLdsA = 8192, kLdsB = 4096;   // floats of the two LDS buffers
constexpr int kPartials = 256;              // blocks per item of the first min / max stage

size_t dtype_bytes(int dt) { return dt == MI_PS_U8 ? 1 : dt == MI_PS_U16 ? 2 : 4; }
bool dtype_ok(int dt) { return dt == MI_PS_U8 || dt == MI_PS_U16 || dt == MI_PS_F32; }

// ---------------------------------------------------------------------------------------------------------------------------------
// halving chain

struct HalveArgs {
    int ny, nx, hy, hx;
    int ky, kx;
    int tile_y, tile_x;     // of the halved plane, powers of two
    int pre_y;              // 1: the chain starts with a y halving, done on the two rows a lane loads
    int pre_y_method;
    int pre_x;              // x halvings done on the lane's registers
    int pre_x_method[4];
    int nrest;              // steps in LDS
    unsigned char rest_axis[MI_ISO_MAX_STEPS], rest_method[MI_ISO_MAX_STEPS];
};

__device__ inline float halve_op(float a, float b, int method) { return method == MI_HALVE_MAX ? fmaxf(a, b) : (a + b) * 0.5f; }

// V samples of row r from column c as floats (zeros past the slice); differ |= a loaded sample is not `first`
template <class T, bool VEC>
__device__ inline void load_run(const T* __restrict__ src, int ny, int nx, i64 r, i64 c, T first, float* v, bool& differ) {
    constexpr int V = 16 / (int)sizeof(T);
    if (r >= ny || c >= nx) {
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = 0.0f;
        return;
    }
    const T* p = src + r * nx + c;
    if (VEC) {   // nx is a multiple of V and the slices are 16-byte aligned: the run is inside the row
        union { uint4 q; T t[V]; } u;
        u.q = *reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            differ |= u.t[j] != first;
            v[j] = (float)u.t[j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            if (c + j < nx) {
                const T s = p[j];
                differ |= s != first;
                v[j] = (float)s;
            } else {
                v[j] = 0.0f;
            }
        }
    }
}

template <class T, bool VEC>
__global__ void __launch_bounds__(kThreads) halve_kernel(const T* __restrict__ in, i64 slice_px, HalveArgs a, float* __restrict__ out,
                                                         int* __restrict__ differs) {
    constexpr int V = 16 / (int)sizeof(T);
    __shared__ float buf_a[kLdsA];
    __shared__ float buf_b[kLdsB];
    const int t = threadIdx.x;
    const i64 slice = blockIdx.z;
    const T* src = in + slice * slice_px;
    const T first = src[0];
    const int rows = a.tile_y << a.ky, cols = a.tile_x << a.kx;   // the source block
    const i64 r0 = (i64)blockIdx.y * rows, c0 = (i64)blockIdx.x * cols;
    const int unit_rows = rows >> a.pre_y, unit_cols = cols / V;
    const int keep = V >> a.pre_x;            // floats a lane hands to LDS
    int w = cols >> a.pre_x, h = unit_rows;   // extents of the block in LDS
    bool differ = false;
    for (int u = t; u < unit_rows * unit_cols; u += kThreads) {
        const int ur = u / unit_cols, uc = u - ur * unit_cols;
        const i64 c = c0 + (i64)uc * V;
        float v[V];
        if (a.pre_y) {
            float v1[V];
            load_run<T, VEC>(src, a.ny, a.nx, r0 + 2 * (i64)ur, c, first, v, differ);
            load_run<T, VEC>(src, a.ny, a.nx, r0 + 2 * (i64)ur + 1, c, first, v1, differ);
#pragma unroll
            for (int j = 0; j < V; ++j) v[j] = halve_op(v[j], v1[j], a.pre_y_method);
        } else {
            load_run<T, VEC>(src, a.ny, a.nx, r0 + ur, c, first, v, differ);
        }
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            if (s < a.pre_x) {
#pragma unroll
                for (int j = 0; j < (V >> (s + 1)); ++j) v[j] = halve_op(v[2 * j], v[2 * j + 1], a.pre_x_method[s]);
            }
        }
        float* dst = buf_a + ur * w + uc * keep;
#pragma unroll
        for (int j = 0; j < V; ++j)
            if (j < keep) dst[j] = v[j];
    }
    if (differ) differs[slice] = 1;   // every writer stores the same value
    __syncthreads();
    float* cur = buf_a;
    float* nxt = buf_b;
    for (int s = 0; s < a.nrest; ++s) {
        const int method = a.rest_method[s];
        if (a.rest_axis[s] == 0) {
            const int h2 = h >> 1;
            for (int i = t; i < h2 * w; i += kThreads) {
                const int y = i / w, x = i - y * w;
                nxt[i] = halve_op(cur[(2 * y) * w + x], cur[(2 * y + 1) * w + x], method);
            }
            h = h2;
        } else {
            const int w2 = w >> 1;
            for (int i = t; i < h * w2; i += kThreads) nxt[i] = halve_op(cur[2 * i], cur[2 * i + 1], method);   // rows are even: pairs never straddle
            w = w2;
        }
        __syncthreads();
        float* tmp = cur;
        cur = nxt;
        nxt = tmp;
    }
    // h == tile_y, w == tile_x
    const i64 oy0 = (i64)blockIdx.y * a.tile_y, ox0 = (i64)blockIdx.x * a.tile_x;
    float* plane = out + slice * ((i64)a.hy * a.hx);
    for (int i = t; i < h * w; i += kThreads) {
        const int y = i / w, x = i - y * w;
        if (oy0 + y < a.hy && ox0 + x < a.hx) plane[(oy0 + y) * a.hx + ox0 + x] = cur[i];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// min / max of `items` dense float32 arrays of `count` samples: partial [items][kPartials][2], then mm [items][2]

__device__ inline void block_minmax(float& lo, float& hi) {
    __shared__ float s_lo[kThreads / 64], s_hi[kThreads / 64];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, d));
        hi = fmaxf(hi, __shfl_xor(hi, d));
    }
    if ((threadIdx.x & 63) == 0) {
        s_lo[threadIdx.x >> 6] = lo;
        s_hi[threadIdx.x >> 6] = hi;
    }
    __syncthreads();
    lo = s_lo[0];
    hi = s_hi[0];
#pragma unroll
    for (int k = 1; k < kThreads / 64; ++k) {
        lo = fminf(lo, s_lo[k]);
        hi = fmaxf(hi, s_hi[k]);
    }
}

__global__ void __launch_bounds__(kThreads) minmax_partial_kernel(const float* __restrict__ in, i64 count, float* __restrict__ partial) {
    const float* src = in + (i64)blockIdx.y * count;
    float lo = src[0], hi = lo;
    for (i64 i = (i64)blockIdx.x * kThreads + threadIdx.x; i < count; i += (i64)gridDim.x * kThreads) {
        const float v = src[i];
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        float* p = partial + ((i64)blockIdx.y * kPartials + blockIdx.x) * 2;
        p[0] = lo;
        p[1] = hi;
    }
}

__global__ void __launch_bounds__(kThreads) minmax_final_kernel(const float* __restrict__ partial, int blocks, float* __restrict__ mm) {
    const float* p = partial + (i64)blockIdx.x * kPartials * 2;
    float lo = p[0], hi = p[1];
    for (int i = threadIdx.x; i < blocks; i += kThreads) {
        lo = fminf(lo, p[2 * i]);
        hi = fmaxf(hi, p[2 * i + 1]);
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        mm[2 * blockIdx.x] = lo;
        mm[2 * blockIdx.x + 1] = hi;
    }
}

int launch_minmax(hipStream_t st, const float* in, i64 count, int items, float* partial, float* mm) {
    const int blocks = (int)std::min<i64>(kPartials, (count + kThreads * 8 - 1) / (kThreads * 8));
    hipLaunchKernelGGL(minmax_partial_kernel, dim3(blocks, items), dim3(kThreads), 0, st, in, count, partial);
    MI_TRY(launch_check("minmax_partial_kernel"));
    hipLaunchKernelGGL(minmax_final_kernel, dim3(items), dim3(kThreads), 0, st, partial, blocks, mm);
    return launch_check("minmax_final_kernel");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// resize

// scipy's 'mirror': d c b | a b c d | c b a, of any reach
__device__ inline int mirror(i64 i, int n) {
    if (n == 1) return 0;
    const i64 p = 2 * ((i64)n - 1);
    i %= p;
    if (i < 0) i += p;
    return (int)(i < n ? i : p - i);
}

// one axis of gaussian_filter on [outer][n][inner]
__global__ void __launch_bounds__(kThreads) gauss_axis_kernel(const float* __restrict__ in, float* __restrict__ out, i64 total, int n, i64 inner,
                                                              const double* __restrict__ taps, int radius) {
    const i64 idx = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= total) return;
    const i64 k = idx % inner, oi = idx / inner;
    const int i = (int)(oi % n);
    const i64 base = (oi - i) * inner + k;
    double acc = 0.0;
    for (int d = -radius; d <= radius; ++d) acc += taps[d + radius] * (double)in[base + (i64)mirror((i64)i + d, n) * inner];
    out[idx] = (float)acc;
}

struct Interp {
    int in[3], out[3];   // z, y, x
    double zoom[3];      // in / out
};

// scipy.ndimage.zoom(order=1, mode='mirror', grid_mode=True) of `items` arrays; clip to mm[item]; zeros where differs[item] == 0
__global__ void __launch_bounds__(kThreads) interp_kernel(const float* __restrict__ in, float* __restrict__ out, Interp g, i64 per_item,
                                                          const float* __restrict__ mm, const int* __restrict__ differs) {
    const i64 idx = (i64)blockIdx.x * kThreads + threadIdx.x;
    if (idx >= per_item) return;
    const i64 item = blockIdx.y;
    float* dst = out + item * per_item;
    if (differs && !differs[item]) {
        dst[idx] = 0.0f;
        return;
    }
    const int x = (int)(idx % g.out[2]), y = (int)((idx / g.out[2]) % g.out[1]), z = (int)(idx / ((i64)g.out[2] * g.out[1]));
    const int o[3] = {z, y, x};
    int i0[3], i1[3];
    double f[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double c = ((double)o[a] + 0.5) * g.zoom[a] - 0.5;
        const double fl = floor(c);
        f[a] = c - fl;
        i0[a] = mirror((i64)fl, g.in[a]);
        i1[a] = mirror((i64)fl + 1, g.in[a]);
    }
    const float* src = in + item * ((i64)g.in[0] * g.in[1] * g.in[2]);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bz = c >> 2, by = (c >> 1) & 1, bx = c & 1;
        const double wgt = (bz ? f[0] : 1.0 - f[0]) * (by ? f[1] : 1.0 - f[1]) * (bx ? f[2] : 1.0 - f[2]);
        if (wgt != 0.0) acc += wgt * (double)src[((i64)(bz ? i1[0] : i0[0]) * g.in[1] + (by ? i1[1] : i0[1])) * g.in[2] + (bx ? i1[2] : i0[2])];
    }
    float v = (float)acc;
    if (mm) v = fminf(fmaxf(v, mm[2 * item]), mm[2 * item + 1]);
    dst[idx] = v;
}

// one axis of a resize: sigma, radius and scipy's taps (_gaussian_kernel1d, double)
struct AxisFilter {
    double sigma = 0.0;
    int radius = 0;
    std::vector<double> taps;
};

int make_filter(int n_in, int n_out, AxisFilter& f) {
    const double factor = (double)n_in / (double)n_out;
    f.sigma = std::max(0.0, (factor - 1.0) / 2.0);
    f.radius = 0;
    f.taps.clear();
    if (f.sigma <= 1e-15) {
        f.sigma = f.sigma > 0.0 ? f.sigma : 0.0;
        return MI_OK;
    }
    f.radius = (int)(4.0 * f.sigma + 0.5);
    if (f.radius > MI_ISO_MAX_RADIUS)
        return fail(MI_ERR_UNSUPPORTED, "mi_resize_antialias: %d -> %d samples needs a Gaussian radius of %d (at most %d is built)", n_in, n_out,
                    f.radius, MI_ISO_MAX_RADIUS);
    f.taps.resize(2 * f.radius + 1);
    double sum = 0.0;
    for (int i = -f.radius; i <= f.radius; ++i) sum += f.taps[i + f.radius] = std::exp(-0.5 / (f.sigma * f.sigma) * (double)i * (double)i);
    for (double& w : f.taps) w /= sum;
    return MI_OK;
}

// resize of `items` arrays of shape in[3] -> out[3] (z, y, x).  tmp_a / tmp_b: each items * prod(in) floats; taps_dev: the device
// taps of the three axes one after the other (offsets taps_off); mm: items pairs; partial: items * kPartials pairs.
int run_resize(hipStream_t st, const float* src, int items, const int* in, const int* out, const AxisFilter* filt, const double* taps_dev,
               const int* taps_off, float* tmp_a, float* tmp_b, float* partial, float* mm, const int* differs, float* dst) {
    const i64 in_count = (i64)in[0] * in[1] * in[2], out_count = (i64)out[0] * out[1] * out[2];
    MI_TRY(launch_minmax(st, src, in_count, items, partial, mm));
    bool any = false;
    for (int a = 0; a < 3; ++a) any |= (double)in[a] / (double)out[a] > 1.0;
    const float* cur = src;
    if (any) {
        const i64 total = in_count * items;
        for (int a = 0; a < 3; ++a) {
            if (filt[a].taps.empty()) continue;
            const i64 inner = a == 0 ? (i64)in[1] * in[2] : a == 1 ? in[2] : 1;
            float* to = cur == tmp_a ? tmp_b : tmp_a;
            hipLaunchKernelGGL(gauss_axis_kernel, dim3(cdiv((size_t)total, kThreads)), dim3(kThreads), 0, st, cur, to, total, in[a], inner,
                               taps_dev + taps_off[a], filt[a].radius);
            MI_TRY(launch_check("gauss_axis_kernel"));
            cur = to;
        }
    }
    Interp g;
    for (int a = 0; a < 3; ++a) {
        g.in[a] = in[a];
        g.out[a] = out[a];
        g.zoom[a] = (double)in[a] / (double)out[a];
    }
    hipLaunchKernelGGL(interp_kernel, dim3(cdiv((size_t)out_count, kThreads), items), dim3(kThreads), 0, st, cur, dst, g, out_count, mm, differs);
    return launch_check("interp_kernel");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// z reduction

__device__ inline void store_plane(void* out, int dt, int src_u8, i64 o, float v) {
    if (dt == MI_PS_F32) {
        static_cast<float*>(out)[o] = v;
        return;
    }
    if (dt == MI_PS_U8 && src_u8) {   // numpy's astype(uint8) of values inside 0 .. 255
        static_cast<uint8_t*>(out)[o] = (uint8_t)fminf(fmaxf(v, 0.0f), 255.0f);
        return;
    }
    const unsigned wide = (unsigned)(v > 0.0f ? (v < 65535.0f ? v : 65535.0f) : 0.0f);   // NaN -> 0
    if (dt == MI_PS_U16) {
        static_cast<uint16_t*>(out)[o] = (uint16_t)wide;
        return;
    }
    unsigned b = wide >> 8;
    b = b > 255u ? 255u : b;
    if (wide > 0 && b == 0) b = 1;
    static_cast<uint8_t*>(out)[o] = (uint8_t)b;
}

__global__ void __launch_bounds__(kThreads) reduce_z_kernel(float* __restrict__ stack, int n, i64 plane_px, int rounds, const float* __restrict__ mm,
                                                            void* __restrict__ out, int out_dt, int src_u8, int* __restrict__ uniform) {
    const i64 p = (i64)blockIdx.x * kThreads + threadIdx.x;
    const bool same = mm[0] == mm[1];
    if (p == 0 && uniform) *uniform = same ? 1 : 0;
    if (p >= plane_px) return;
    if (same) {
        store_plane(out, out_dt, src_u8, p, 0.0f);
        return;
    }
    int m = n;
    for (int r = 0; r < rounds && m > 1; ++r) {
        const int m2 = (m + 1) >> 1;
        for (int i = 0; i < m2; ++i) {
            const float a = stack[(i64)(2 * i) * plane_px + p];
            const float b = 2 * i + 1 < m ? stack[(i64)(2 * i + 1) * plane_px + p] : 0.0f;
            stack[(i64)i * plane_px + p] = halve_op(a, b, (r & 1) ? MI_HALVE_MEAN : MI_HALVE_MAX);
        }
        m = m2;
    }
    store_plane(out, out_dt, src_u8, p, stack[p]);
}

int check_z(int n, int rounds) {
    MI_REQUIRE(n >= 1 && rounds >= 0, "mi_isodown: %d planes, %d rounds", n, rounds);
    int m = n;
    for (int r = 0; r < rounds && m > 1; ++r) m = (m + 1) / 2;
    MI_REQUIRE(m == 1, "mi_isodown: %d rounds along z leave %d of %d planes (the reference stops on this geometry)", rounds, m, n);
    return MI_OK;
}

int launch_reduce_z(hipStream_t st, float* stack, int n, i64 plane_px, int rounds, float* partial, float* mm, void* plane, int out_dt, int src_u8,
                    int* uniform) {
    MI_TRY(launch_minmax(st, stack, (i64)n * plane_px, 1, partial, mm));
    hipLaunchKernelGGL(reduce_z_kernel, dim3(cdiv((size_t)plane_px, kThreads)), dim3(kThreads), 0, st, stack, n, plane_px, rounds, mm, plane, out_dt,
                       src_u8, uniform);
    return launch_check("reduce_z_kernel");
}

// ---------------------------------------------------------------------------------------------------------------------------------
// plan

struct Plan {
    int dev = 0, src_dt = 0;
    mi_isodown_params prm{};
    mi_isodown_info info{};
    HalveArgs ha{};
    AxisFilter filt[3];
    int taps_off[3] = {0, 0, 0};
    DevBuf taps, scratch;
    i64 cap = 0;
    // offsets into scratch (bytes), for cap slices
    size_t off_halved = 0, off_tmp_a = 0, off_tmp_b = 0, off_stack = 0, off_flags = 0, off_mm = 0, off_partial = 0;
};

// tile and register steps of the halving kernel for samples of `bytes`
int shape_halve(const mi_isodown_info& I, int bytes, HalveArgs& a) {
    a = HalveArgs{};
    a.ny = I.ny; a.nx = I.nx; a.hy = I.halved_ny; a.hx = I.halved_nx; a.ky = I.ky; a.kx = I.kx;
    const int V = 16 / bytes;
    int s = 0;
    if (s < I.nsteps && I.step_axis[s] == 0) {
        a.pre_y = 1;
        a.pre_y_method = I.step_method[s++];
    }
    while (s < I.nsteps && I.step_axis[s] == 1 && (V >> (a.pre_x + 1)) >= 1 && a.pre_x < 4) a.pre_x_method[a.pre_x++] = I.step_method[s++];
    a.nrest = I.nsteps - s;
    for (int i = 0; i < a.nrest; ++i) {
        a.rest_axis[i] = (unsigned char)I.step_axis[s + i];
        a.rest_method[i] = (unsigned char)I.step_method[s + i];
    }
    if (I.kx > 20 || I.ky > 20) return fail(MI_ERR_UNSUPPORTED, "mi_isodown: %d / %d halvings of one axis", I.ky, I.kx);
    i64 cols = std::max<i64>(1ll << I.kx, 256), rows = 1ll << I.ky;
    auto lds = [&](i64 r, i64 c) { return (r >> a.pre_y) * (c >> a.pre_x); };
    while (rows < 64 && lds(rows * 2, cols) <= kLdsA) rows *= 2;
    while (lds(rows, cols) > kLdsA && cols > std::max<i64>(1ll << I.kx, 16)) cols /= 2;
    if (lds(rows, cols) > kLdsA)
        return fail(MI_ERR_UNSUPPORTED, "mi_isodown: a source block of %lld x %lld samples behind one halved sample does not fit the kernel's tile",
                    1ll << I.ky, 1ll << I.kx);
    a.tile_y = (int)(rows >> I.ky);
    a.tile_x = (int)(cols >> I.kx);
    return MI_OK;
}

int derive(int ny, int nx, double vy, double vx, double target, int alternating, mi_isodown_info& I) {
    MI_REQUIRE(ny > 0 && nx > 0, "mi_isodown: slice shape (%d, %d)", ny, nx);
    MI_REQUIRE(vy > 0.0 && vx > 0.0 && target > 0.0 && std::isfinite(vy) && std::isfinite(vx) && std::isfinite(target),
               "mi_isodown: voxel (%g, %g), target %g", vy, vx, target);
    I = mi_isodown_info{};
    I.ny = ny; I.nx = nx;
    const double ry = target / vy, rx = target / vx;
    const double ty = std::nearbyint((double)ny / ry), tx = std::nearbyint((double)nx / rx);   // numpy.round: half to even
    MI_REQUIRE(ty >= 1.0 && tx >= 1.0, "mi_isodown: the target shape of a (%d, %d) slice rounds to (%g, %g)", ny, nx, ty, tx);
    MI_REQUIRE(ty < 2147483647.0 && tx < 2147483647.0, "mi_isodown: target shape (%g, %g)", ty, tx);
    I.target_ny = (int)ty; I.target_nx = (int)tx;
    const double fy = std::floor(std::sqrt(ry)), fx = std::floor(std::sqrt(rx));
    MI_REQUIRE(fy <= 1000.0 && fx <= 1000.0, "mi_isodown: %g / %g halving rounds", fy, fx);
    I.rounds_y = (int)fy; I.rounds_x = (int)fx;
    // the shorter list of rounds is padded with "none"; without alternation every round, the padding included, is mean / mean
    const int most = std::max(I.rounds_y, I.rounds_x);
    const int use_y = alternating ? I.rounds_y : most, use_x = alternating ? I.rounds_x : most;
    int h = ny, w = nx;
    for (int r = 0; r < most; ++r) {
        if (r < use_y && (h + 1) / 2 >= I.target_ny) {
            if (I.nsteps == MI_ISO_MAX_STEPS) return fail(MI_ERR_UNSUPPORTED, "mi_isodown: more than %d halvings", MI_ISO_MAX_STEPS);
            I.step_axis[I.nsteps] = 0;
            I.step_method[I.nsteps] = !alternating ? MI_HALVE_MEAN : (r % 2 == 0 ? MI_HALVE_MAX : MI_HALVE_MEAN);
            I.step_extent[I.nsteps++] = h;
            h = (h + 1) / 2;
            ++I.ky;
        }
        if (r < use_x && (w + 1) / 2 >= I.target_nx) {
            if (I.nsteps == MI_ISO_MAX_STEPS) return fail(MI_ERR_UNSUPPORTED, "mi_isodown: more than %d halvings", MI_ISO_MAX_STEPS);
            I.step_axis[I.nsteps] = 1;
            I.step_method[I.nsteps] = !alternating ? MI_HALVE_MEAN : (r % 2 == 0 ? MI_HALVE_MEAN : MI_HALVE_MAX);
            I.step_extent[I.nsteps++] = w;
            w = (w + 1) / 2;
            ++I.kx;
        }
    }
    I.halved_ny = h; I.halved_nx = w;
    AxisFilter f;
    MI_TRY(make_filter(h, I.target_ny, f));
    I.sigma_y = f.sigma; I.radius_y = f.radius; I.taps_y = (int)f.taps.size();
    MI_TRY(make_filter(w, I.target_nx, f));
    I.sigma_x = f.sigma; I.radius_x = f.radius; I.taps_x = (int)f.taps.size();
    HalveArgs a;
    if (shape_halve(I, 2, a) == MI_OK) {   // (0, 0): the source block behind one halved sample is larger than the kernel's tile; no plan
        I.tile_ny = a.tile_y; I.tile_nx = a.tile_x; I.lds_steps = a.nrest;
    }
    const size_t halved = ((size_t)h * w * 4 + 15) / 16 * 16, plane = ((size_t)I.target_ny * I.target_nx * 4 + 15) / 16 * 16;
    I.scratch_bytes_per_slice = 3 * halved + plane + 16 + 16 + (size_t)kPartials * 8;
    return MI_OK;
}

template <class T>
int launch_halve_t(hipStream_t st, const Plan& P, const void* in, int cnt, float* halved, int* differs) {
    constexpr int V = 16 / (int)sizeof(T);
    const i64 slice_px = (i64)P.info.ny * P.info.nx;
    const bool vec = P.info.nx % V == 0 && slice_px % V == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    const dim3 grid(cdiv(P.info.halved_nx, P.ha.tile_x), cdiv(P.info.halved_ny, P.ha.tile_y), cnt);
    MI_REQUIRE(grid.y <= 65535u, "mi_isodown: %u tile rows", grid.y);
    if (vec) hipLaunchKernelGGL((halve_kernel<T, true>), grid, dim3(kThreads), 0, st, static_cast<const T*>(in), slice_px, P.ha, halved, differs);
    else hipLaunchKernelGGL((halve_kernel<T, false>), grid, dim3(kThreads), 0, st, static_cast<const T*>(in), slice_px, P.ha, halved, differs);
    return launch_check("halve_kernel");
}

int launch_halve(hipStream_t st, const Plan& P, const void* in, int cnt, float* halved, int* differs) {
    MI_HIP(hipMemsetAsync(differs, 0, sizeof(int) * (size_t)cnt, st));
    if (P.src_dt == MI_PS_U8) return launch_halve_t<uint8_t>(st, P, in, cnt, halved, differs);
    if (P.src_dt == MI_PS_U16) return launch_halve_t<uint16_t>(st, P, in, cnt, halved, differs);
    return launch_halve_t<float>(st, P, in, cnt, halved, differs);
}

size_t up16(size_t n) { return (n + 15) / 16 * 16; }

int ensure_scratch(Plan& P, hipStream_t st, i64 want) {
    if (want <= P.cap) return MI_OK;
    MI_HIP(hipStreamSynchronize(st));   // work of an earlier call may still use the smaller scratch
    P.cap = 0;
    const size_t halved = up16((size_t)P.info.halved_ny * P.info.halved_nx * 4 * (size_t)want);
    const size_t stack = up16((size_t)P.info.target_ny * P.info.target_nx * 4 * (size_t)want);
    size_t o = 0;
    P.off_halved = o; o += halved;
    P.off_tmp_a = o; o += halved;
    P.off_tmp_b = o; o += halved;
    P.off_stack = o; o += stack;
    P.off_flags = o; o += up16(sizeof(int) * (size_t)want);
    P.off_mm = o; o += up16(8 * (size_t)want);
    P.off_partial = o; o += (size_t)kPartials * 8 * (size_t)want;
    MI_TRY(P.scratch.alloc(o));
    P.cap = want;
    return MI_OK;
}

// planes of cnt <= cap slices into `planes`
int run_planes(Plan& P, hipStream_t st, const void* in, int cnt, float* planes) {
    char* s = P.scratch.as<char>();
    float* halved = reinterpret_cast<float*>(s + P.off_halved);
    int* differs = reinterpret_cast<int*>(s + P.off_flags);
    MI_TRY(launch_halve(st, P, in, cnt, halved, differs));
    const int shape_in[3] = {1, P.info.halved_ny, P.info.halved_nx}, shape_out[3] = {1, P.info.target_ny, P.info.target_nx};
    return run_resize(st, halved, cnt, shape_in, shape_out, P.filt, P.taps.as<double>(), P.taps_off, reinterpret_cast<float*>(s + P.off_tmp_a),
                      reinterpret_cast<float*>(s + P.off_tmp_b), reinterpret_cast<float*>(s + P.off_partial), reinterpret_cast<float*>(s + P.off_mm),
                      differs, planes);
}

int upload_taps(const AxisFilter* filt, int* off, DevBuf& buf) {
    std::vector<double> all;
    for (int a = 0; a < 3; ++a) {
        off[a] = (int)all.size();
        all.insert(all.end(), filt[a].taps.begin(), filt[a].taps.end());
    }
    if (all.empty()) all.push_back(1.0);
    MI_TRY(buf.alloc(all.size() * sizeof(double)));
    MI_HIP(hipMemcpy(buf.p, all.data(), all.size() * sizeof(double), hipMemcpyHostToDevice));
    return MI_OK;
}

}  // namespace
}  // namespace mi

using mi::Plan;

extern "C" int mi_isodown_derive(int ny, int nx, double voxel_y, double voxel_x, double target_voxel, int alternating, mi_isodown_info* info) {
    MI_REQUIRE(info, "mi_isodown_derive: null pointer");
    return mi::derive(ny, nx, voxel_y, voxel_x, target_voxel, alternating, *info);
}

extern "C" int mi_isodown_plan_create(int dev, int ny, int nx, int src_dtype, const mi_isodown_params* params, void** plan) {
    MI_REQUIRE(params && plan, "mi_isodown_plan_create: null pointer");
    *plan = nullptr;
    MI_REQUIRE(mi::dtype_ok(src_dtype) && mi::dtype_ok(params->out_dtype), "mi_isodown_plan_create: dtype %d -> %d", src_dtype, params->out_dtype);
    MI_REQUIRE(params->z_rounds >= 0, "mi_isodown_plan_create: z_rounds %d", params->z_rounds);
    MI_TRY(mi::use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    P->src_dt = src_dtype;
    P->prm = *params;
    if (P->prm.max_group <= 0) P->prm.max_group = 16;
    int rc = mi::derive(ny, nx, params->voxel_y, params->voxel_x, params->target_voxel, params->alternating, P->info);
    if (rc == MI_OK) rc = mi::shape_halve(P->info, (int)mi::dtype_bytes(src_dtype), P->ha);
    if (rc == MI_OK) {
        P->info.tile_ny = P->ha.tile_y; P->info.tile_nx = P->ha.tile_x; P->info.lds_steps = P->ha.nrest;
        rc = mi::make_filter(P->info.halved_ny, P->info.target_ny, P->filt[1]);
    }
    if (rc == MI_OK) rc = mi::make_filter(P->info.halved_nx, P->info.target_nx, P->filt[2]);
    if (rc == MI_OK) rc = mi::upload_taps(P->filt, P->taps_off, P->taps);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    *plan = P;
    return MI_OK;
}

extern "C" int mi_isodown_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_isodown_plan_info(void* plan, mi_isodown_info* info) {
    MI_REQUIRE(plan && info, "mi_isodown_plan_info: null pointer");
    *info = static_cast<Plan*>(plan)->info;
    return MI_OK;
}

extern "C" int mi_isodown_halve(void* plan, void* stream, const void* in, int64_t count, float* halved, int* differs) {
    MI_REQUIRE(plan && in && halved && differs, "mi_isodown_halve: null pointer");
    MI_REQUIRE(count >= 0 && count <= 65535, "mi_isodown_halve: count %lld", (long long)count);
    if (count == 0) return MI_OK;
    Plan& P = *static_cast<Plan*>(plan);
    MI_TRY(mi::use_device(P.dev));
    return mi::launch_halve(mi::as_stream(stream), P, in, (int)count, halved, differs);
}

extern "C" int mi_isodown_planes(void* plan, void* stream, const void* in, int64_t count, float* planes) {
    MI_REQUIRE(plan && in && planes, "mi_isodown_planes: null pointer");
    MI_REQUIRE(count >= 0, "mi_isodown_planes: count %lld", (long long)count);
    if (count == 0) return MI_OK;
    Plan& P = *static_cast<Plan*>(plan);
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    MI_TRY(mi::ensure_scratch(P, st, std::min<int64_t>(count, P.prm.max_group)));
    const size_t slice_bytes = (size_t)P.info.ny * P.info.nx * mi::dtype_bytes(P.src_dt), plane_px = (size_t)P.info.target_ny * P.info.target_nx;
    for (int64_t s0 = 0; s0 < count; s0 += P.cap) {
        const int cnt = (int)std::min<int64_t>(P.cap, count - s0);
        MI_TRY(mi::run_planes(P, st, static_cast<const char*>(in) + (size_t)s0 * slice_bytes, cnt, planes + (size_t)s0 * plane_px));
    }
    return MI_OK;
}

extern "C" int mi_isodown_run(void* plan, void* stream, const void* in, int64_t count, void* plane, int* uniform) {
    MI_REQUIRE(plan && in && plane, "mi_isodown_run: null pointer");
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(count >= 1 && count <= P.prm.max_group, "mi_isodown_run: a group of %lld slices (the plan holds scratch for 1 .. %d)", (long long)count,
               P.prm.max_group);
    MI_TRY(mi::check_z((int)count, P.prm.z_rounds));
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    MI_TRY(mi::ensure_scratch(P, st, count));
    char* s = P.scratch.as<char>();
    float* stack = reinterpret_cast<float*>(s + P.off_stack);
    MI_TRY(mi::run_planes(P, st, in, (int)count, stack));
    return mi::launch_reduce_z(st, stack, (int)count, (mi::i64)P.info.target_ny * P.info.target_nx, P.prm.z_rounds,
                               reinterpret_cast<float*>(s + P.off_partial), reinterpret_cast<float*>(s + P.off_mm), plane, P.prm.out_dtype,
                               P.src_dt == MI_PS_U8, uniform);
}

extern "C" int mi_isodown_reduce_z(int dev, void* stream, float* stack, int n, int ny, int nx, int rounds, int src_is_u8, int out_dtype, void* plane,
                                   int* uniform) {
    MI_REQUIRE(stack && plane, "mi_isodown_reduce_z: null pointer");
    MI_REQUIRE(ny > 0 && nx > 0 && mi::dtype_ok(out_dtype), "mi_isodown_reduce_z: planes of (%d, %d), dtype %d", ny, nx, out_dtype);
    MI_TRY(mi::check_z(n, rounds));
    MI_TRY(mi::use_device(dev));
    hipStream_t st = mi::as_stream(stream);
    mi::DevBuf work;
    MI_TRY(work.alloc((size_t)mi::kPartials * 8 + 16));
    float* partial = work.as<float>();
    MI_TRY(mi::launch_reduce_z(st, stack, n, (mi::i64)ny * nx, rounds, partial, partial + 2 * mi::kPartials, plane, out_dtype, src_is_u8, uniform));
    MI_HIP(hipStreamSynchronize(st));   // the work buffer goes back to the pool
    return MI_OK;
}

extern "C" int mi_resize_antialias(int dev, void* stream, const float* in, int ndim, const int* in_shape, const int* out_shape, float* out) {
    MI_REQUIRE(in && out && in_shape && out_shape, "mi_resize_antialias: null pointer");
    MI_REQUIRE(ndim == 2 || ndim == 3, "mi_resize_antialias: ndim %d (2 and 3 are built)", ndim);
    int si[3] = {1, 1, 1}, so[3] = {1, 1, 1};
    for (int a = 0; a < ndim; ++a) {
        si[3 - ndim + a] = in_shape[a];
        so[3 - ndim + a] = out_shape[a];
        MI_REQUIRE(in_shape[a] >= 1 && out_shape[a] >= 1, "mi_resize_antialias: extent %d -> %d", in_shape[a], out_shape[a]);
    }
    mi::AxisFilter filt[3];
    for (int a = 0; a < 3; ++a) MI_TRY(mi::make_filter(si[a], so[a], filt[a]));
    MI_TRY(mi::use_device(dev));
    hipStream_t st = mi::as_stream(stream);
    mi::DevBuf taps, work;
    int off[3];
    MI_TRY(mi::upload_taps(filt, off, taps));
    const size_t count = mi::up16((size_t)si[0] * si[1] * si[2] * 4);
    MI_TRY(work.alloc(2 * count + (size_t)mi::kPartials * 8 + 16));
    char* w = work.as<char>();
    float* partial = reinterpret_cast<float*>(w + 2 * count);
    MI_TRY(mi::run_resize(st, in, 1, si, so, filt, taps.as<double>(), off, reinterpret_cast<float*>(w), reinterpret_cast<float*>(w + count), partial,
                          partial + 2 * mi::kPartials, nullptr, out));
    MI_HIP(hipStreamSynchronize(st));   // the scratch goes back to the pool
    return MI_OK;
}
