// mi_align.h: channel alignment and the RGB composite of align_images.py on the device.
//   mi_sobel2d_f32           get_gradient (process_images.py:310-317): skimage.filters.sobel of a float32 plane
//   mi_ecc_prepare           findTransformECC before its loop (process_images.py:804-812): 5 x 5 Gaussian, central differences
//   mi_ecc_sums              the 15 sums of one forward-additive ECC iteration (Evangelidis & Psarakis, PAMI 2008) at a translation
//   mi_ecc_translation_run   the loop: sums, 2 x 2 solve and update on the device, the state read back once per batch
//   mi_channel_composite     process_single_big_image (align_images.py:271-338): pad, roll, roll, trim, stack, astype as one index map
// The restatement fixes the rounding of every float32 operation per pixel (separate multiply and add), so
// contraction is off for the whole file, for the reason thresholds.hip gives: hipcc contracts by default and an FMA moves a blurred
// sample or a bilinear sample by an ulp.  The sums are float64 sums of products of float32 values (exact products), reduced in a
// fixed order without floating-point atomics: two runs give equal bits.
#include <cmath>
#include <cstdint>

#include "mi_align.h"
#include "mi_internal.h"

#pragma clang fp contract(off)

namespace mi {
namespace {

using i64 = long long;
using u64 = unsigned long long;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kQuad = 4;   // output pixels of one row per thread and step: their 2 x 5 taps per plane are shared

// scipy's `reflect` (d c b a | a b c d) and OpenCV's BORDER_REFLECT_101 (d c b | a b c d) for an index at most 2 outside 0 .. n - 1
__device__ __forceinline__ int reflect_edge(int i, int n) { return i < 0 ? -i - 1 : (i >= n ? 2 * n - i - 1 : i); }
__device__ __forceinline__ int reflect_101(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - i - 2 : i); }

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_sobel2d_f32: one thread per pixel, the 3 x 3 neighbourhood from the cache.  The planes are the mid-planes of a down-sampled
// volume and the pass runs three times per outer iteration of align_images: it is not tuned.

__global__ void __launch_bounds__(kThreads) sobel_kernel(const float* in, int ny, int nx, float* out) {
    const i64 n = (i64)ny * nx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int y = (int)(i / nx), x = (int)(i - (i64)y * nx);
        const int ym = min(reflect_edge(y - 1, ny), ny - 1), yp = min(reflect_edge(y + 1, ny), ny - 1);
        const int xm = min(reflect_edge(x - 1, nx), nx - 1), xp = min(reflect_edge(x + 1, nx), nx - 1);
        const float* rm = in + (i64)ym * nx;
        const float* r0 = in + (i64)y * nx;
        const float* rp = in + (i64)yp * nx;
        const double mm = rm[xm], m0 = rm[x], mp = rm[xp], zm = r0[xm], zp = r0[xp], pm = rp[xm], p0 = rp[x], pp = rp[xp];
        // the convolutions in float64, in the order of the restatement, rounded to float32 as scipy.ndimage stores them
        const float h = (float)(((((0.125 * pm + 0.25 * p0) + 0.125 * pp) - 0.125 * mm) - 0.25 * m0) - 0.125 * mp);
        const float v = (float)(((((0.125 * mp + 0.25 * zp) + 0.125 * pp) - 0.125 * mm) - 0.25 * zm) - 0.125 * pm);
        out[i] = sqrtf((h * h + v * v) / 2.0f);
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_ecc_prepare

constexpr float kC1 = 0.0625f, kC4 = 0.25f, kC6 = 0.375f;   // [1, 4, 6, 4, 1] / 16

__device__ __forceinline__ float taps5(float a, float b, float c, float d, float e) {
    return (((kC1 * a + kC4 * b) + kC6 * c) + kC4 * d) + kC1 * e;
}

// blockIdx.y: 0 the template, 1 the subject.  Rows first, each row sum rounded to float32, then the column: the restatement's order.
__global__ void __launch_bounds__(kThreads) blur5_kernel(const float* in0, const float* in1, int ny, int nx, float* out0, float* out1) {
    const float* in = blockIdx.y ? in1 : in0;
    float* out = blockIdx.y ? out1 : out0;
    const i64 n = (i64)ny * nx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int y = (int)(i / nx), x = (int)(i - (i64)y * nx);
        int xs[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) xs[k] = reflect_101(x + k - 2, nx);
        float h[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            const float* r = in + (i64)reflect_101(y + k - 2, ny) * nx;
            h[k] = taps5(r[xs[0]], r[xs[1]], r[xs[2]], r[xs[3]], r[xs[4]]);
        }
        out[i] = taps5(h[0], h[1], h[2], h[3], h[4]);
    }
}

__global__ void __launch_bounds__(kThreads) gradient_kernel(const float* s, int ny, int nx, float* gx, float* gy) {
    const i64 n = (i64)ny * nx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const int y = (int)(i / nx), x = (int)(i - (i64)y * nx);
        const float* r = s + (i64)y * nx;
        gx[i] = 0.5f * r[reflect_101(x + 1, nx)] - 0.5f * r[reflect_101(x - 1, nx)];
        gy[i] = 0.5f * s[(i64)reflect_101(y + 1, ny) * nx + x] - 0.5f * s[(i64)reflect_101(y - 1, ny) * nx + x];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the ECC iteration

// floor of a translation as an integer that cannot overflow the index arithmetic; a NaN becomes the lower bound (every tap outside)
__device__ __forceinline__ int bounded_int(double v) { return (int)fmin(fmax(v, -1.0e9), 1.0e9); }

// k-th of the 5 samples a quad needs from one source row: row[c0 + k], zero outside the row (r_in: the row lies inside the plane)
__device__ __forceinline__ float tap(const float* row, bool r_in, i64 c0, int k, int nx) {
    const i64 c = c0 + k;
    return (r_in && (u64)c < (u64)nx) ? row[c] : 0.0f;
}

// One pass over the four planes: every sum of mi_ecc_sum into one row of MI_ECC_NSUMS doubles per work-group.  The four bilinear
// weights are the same for every pixel of a translation, so a quad of outputs needs two contiguous runs of 5 samples per plane.
// The template is read with one 16-byte load per quad where rows are 16-byte aligned (nx % 4 == 0 and an aligned base), by elements
// otherwise; the taps are read by elements: their alignment moves with floor(tx) and the runs of neighbouring lanes overlap in cache.
__global__ void __launch_bounds__(kThreads) ecc_sums_kernel(const float* t, const float* s, const float* gx, const float* gy, int ny, int nx,
                                                            const mi_ecc_state* st, double tx_arg, double ty_arg, double* rows) {
    __shared__ double part[kWaves][MI_ECC_NSUMS];
    if (st && st->done) return;   // the whole grid: the batch runs out without work
    const double tx = st ? st->tx : tx_arg, ty = st ? st->ty : ty_arg;
    const double flx = floor(tx), fly = floor(ty);
    const int ix = bounded_int(flx), iy = bounded_int(fly);
    const int rx = bounded_int(floor(tx + 0.5)), ry = bounded_int(floor(ty + 0.5));   // the nearest source pixel, for the mask
    const float fx = (float)(tx - flx), fy = (float)(ty - fly);
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy), w10 = (1.0f - fx) * fy, w11 = fx * fy;
    const bool vec_t = (nx % kQuad) == 0 && ((uintptr_t)t & 15u) == 0;

    double acc[MI_ECC_NSUMS];
#pragma unroll
    for (int k = 0; k < MI_ECC_NSUMS; ++k) acc[k] = 0.0;

    const int qx = (nx + kQuad - 1) / kQuad;
    const i64 nquads = (i64)ny * qx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 q = (i64)blockIdx.x * blockDim.x + threadIdx.x; q < nquads; q += stride) {
        const int y = (int)(q / qx), x0 = (int)(q - (i64)y * qx) * kQuad;
        const i64 r0 = (i64)y + iy, r1 = r0 + 1, c0 = (i64)x0 + ix;
        const bool in0 = (u64)r0 < (u64)ny, in1 = (u64)r1 < (u64)ny;
        const i64 o0 = in0 ? r0 * nx : 0, o1 = in1 ? r1 * nx : 0;
        float sa[5], sb[5], xa[5], xb[5], ya[5], yb[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) {
            sa[k] = tap(s + o0, in0, c0, k, nx);
            sb[k] = tap(s + o1, in1, c0, k, nx);
            xa[k] = tap(gx + o0, in0, c0, k, nx);
            xb[k] = tap(gx + o1, in1, c0, k, nx);
            ya[k] = tap(gy + o0, in0, c0, k, nx);
            yb[k] = tap(gy + o1, in1, c0, k, nx);
        }
        float tv[kQuad];
        const float* trow = t + (i64)y * nx + x0;
        if (vec_t) {
            const float4 v = *reinterpret_cast<const float4*>(trow);
            tv[0] = v.x; tv[1] = v.y; tv[2] = v.z; tv[3] = v.w;
        } else {
#pragma unroll
            for (int j = 0; j < kQuad; ++j) tv[j] = x0 + j < nx ? trow[j] : 0.0f;
        }
        const bool my = (u64)((i64)y + ry) < (u64)ny;
#pragma unroll
        for (int j = 0; j < kQuad; ++j) {
            if (x0 + j >= nx) break;
            const float wf = ((w00 * sa[j] + w01 * sa[j + 1]) + w10 * sb[j]) + w11 * sb[j + 1];
            const float gxf = ((w00 * xa[j] + w01 * xa[j + 1]) + w10 * xb[j]) + w11 * xb[j + 1];
            const float gyf = ((w00 * ya[j] + w01 * ya[j + 1]) + w10 * yb[j]) + w11 * yb[j + 1];
            const double w = wf, gxw = gxf, gyw = gyf, tt = tv[j];
            acc[MI_ECC_HXX] += gxw * gxw;
            acc[MI_ECC_HXY] += gxw * gyw;
            acc[MI_ECC_HYY] += gyw * gyw;
            acc[MI_ECC_GXW] += gxw * w;
            acc[MI_ECC_GYW] += gyw * w;
            if (my && (u64)((i64)x0 + j + rx) < (u64)nx) {
                acc[MI_ECC_N] += 1.0;
                acc[MI_ECC_SW] += w;
                acc[MI_ECC_SWW] += w * w;
                acc[MI_ECC_ST] += tt;
                acc[MI_ECC_STT] += tt * tt;
                acc[MI_ECC_SWT] += w * tt;
                acc[MI_ECC_MGX] += gxw;
                acc[MI_ECC_MGY] += gyw;
                acc[MI_ECC_GXT] += gxw * tt;
                acc[MI_ECC_GYT] += gyw * tt;
            }
        }
    }
    // registers -> wave (xor butterfly: the same order for every lane) -> LDS -> one row per work-group
#pragma unroll
    for (int k = 0; k < MI_ECC_NSUMS - 1; ++k)
        for (int d = 32; d >= 1; d >>= 1) acc[k] += __shfl_xor(acc[k], d);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < MI_ECC_NSUMS; ++k) part[wave][k] = acc[k];
    }
    __syncthreads();
    if (threadIdx.x < MI_ECC_NSUMS) {
        double v = part[0][threadIdx.x];
        for (int w = 1; w < kWaves; ++w) v += part[w][threadIdx.x];
        rows[(i64)blockIdx.x * MI_ECC_NSUMS + threadIdx.x] = v;
    }
}

// the rows of all work-groups in index order, one sum per lane (64 threads, one work-group)
__device__ __forceinline__ void total_rows(const double* rows, int groups, double* total) {
    if (threadIdx.x < MI_ECC_NSUMS) {
        double v = 0.0;
        for (int g = 0; g < groups; ++g) v += rows[(i64)g * MI_ECC_NSUMS + threadIdx.x];
        total[threadIdx.x] = v;
    }
}

__global__ void __launch_bounds__(64) ecc_total_kernel(const double* rows, int groups, double* sums) {
    __shared__ double total[MI_ECC_NSUMS];
    total_rows(rows, groups, total);
    __syncthreads();
    if (threadIdx.x < MI_ECC_NSUMS) sums[threadIdx.x] = total[threadIdx.x];
}

__global__ void ecc_init_kernel(mi_ecc_state* st, double tx, double ty, double eps, int iterations) {
    st->tx = tx;
    st->ty = ty;
    st->rho = -1.0;          // findTransformECC's start: the first test |rho - last_rho| >= eps holds
    st->rho_last = -eps;
    st->iteration = 0;
    st->status = MI_ECC_OK;
    st->done = iterations <= 0;
    st->reserved = 0;
}

// One step of the iterate from the totals (DESIGN section 18 has every formula; the means are factored out of the sums)
__global__ void __launch_bounds__(64) ecc_step_kernel(const double* rows, int groups, mi_ecc_state* st, int iterations, double eps) {
    __shared__ double S[MI_ECC_NSUMS];
    if (st->done) return;
    total_rows(rows, groups, S);
    __syncthreads();
    if (threadIdx.x != 0) return;
    const double n = S[MI_ECC_N];
    const double mean_w = S[MI_ECC_SW] / n, mean_t = S[MI_ECC_ST] / n;
    const double wn2 = fmax(S[MI_ECC_SWW] - S[MI_ECC_SW] * mean_w, 0.0);   // ||w_zm||^2 over the mask
    const double tn2 = fmax(S[MI_ECC_STT] - S[MI_ECC_ST] * mean_t, 0.0);
    const double corr = S[MI_ECC_SWT] - S[MI_ECC_SW] * mean_t;             // <t_zm, w_zm>
    const double rho = corr / (sqrt(wn2) * sqrt(tn2));
    st->rho_last = st->rho;
    st->rho = rho;
    st->iteration += 1;
    if (rho != rho) {
        st->status = MI_ECC_NAN;
        st->done = 1;
        return;
    }
    const double ipx = S[MI_ECC_GXW] - mean_w * S[MI_ECC_MGX], ipy = S[MI_ECC_GYW] - mean_w * S[MI_ECC_MGY];
    const double tpx = S[MI_ECC_GXT] - mean_t * S[MI_ECC_MGX], tpy = S[MI_ECC_GYT] - mean_t * S[MI_ECC_MGY];
    const double hxx = S[MI_ECC_HXX], hxy = S[MI_ECC_HXY], hyy = S[MI_ECC_HYY];
    const double det = hxx * hyy - hxy * hxy;
    // a singular Hessian inverts to zeros, as OpenCV's Mat::inv does: the step is zero and the loop ends on rho
    const double ixx = det != 0.0 ? hyy / det : 0.0, ixy = det != 0.0 ? -hxy / det : 0.0, iyy = det != 0.0 ? hxx / det : 0.0;
    const double hix = ixx * ipx + ixy * ipy, hiy = ixy * ipx + iyy * ipy;   // H^-1 ip
    const double lambda_n = wn2 - (ipx * hix + ipy * hiy);
    const double lambda_d = corr - (tpx * hix + tpy * hiy);
    if (!(lambda_d > 0.0)) {
        st->status = MI_ECC_MINIMIZED;
        st->done = 1;
        return;
    }
    const double lambda = lambda_n / lambda_d;
    const double ex = lambda * tpx - ipx, ey = lambda * tpy - ipy;
    st->tx += ixx * ex + ixy * ey;
    st->ty += ixy * ex + iyy * ey;
    if (st->iteration >= iterations || fabs(rho - st->rho_last) < eps) st->done = 1;
}

int sum_groups(int ny, int nx) {
    const i64 quads = (i64)ny * ((nx + kQuad - 1) / kQuad);
    const i64 g = (quads + kThreads - 1) / kThreads;
    return (int)(g < 1 ? 1 : (g > MI_ECC_MAX_GROUPS ? MI_ECC_MAX_GROUPS : g));
}

int check_planes(const char* who, const void* const* planes, int count, int ny, int nx, int least) {
    for (int k = 0; k < count; ++k) {
        MI_REQUIRE(planes[k], "%s: null pointer", who);
        MI_REQUIRE(((uintptr_t)planes[k] % 4) == 0, "%s: float planes must be 4-byte aligned", who);
    }
    MI_REQUIRE(ny >= least && nx >= least && (i64)ny * nx <= (1ll << 40), "%s: ny=%d nx=%d, at least %d each", who, ny, nx, least);
    return MI_OK;
}

unsigned pixel_blocks(i64 n) {
    const i64 b = (n + kThreads - 1) / kThreads;
    return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// mi_channel_composite: bound by reading and writing the TIFF series around it, not by the device; one thread per output pixel,
// which stores its three samples together.  Not tuned.

template <class T> struct Rgb { T c[3]; };

struct Channels { mi_composite_channel c[3]; };

template <class Tin, class Tout>
__global__ void __launch_bounds__(kThreads) composite_kernel(Channels ch, int z0, int n, int ny, int nx, Rgb<Tout>* out) {
    const i64 total = (i64)n * ny * nx;
    const i64 stride = (i64)gridDim.x * blockDim.x;
    for (i64 i = (i64)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const int x = (int)(i % nx);
        const i64 r = i / nx;
        const int y = (int)(r % ny), k = (int)(r / ny);
        Rgb<Tout> px;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const mi_composite_channel& m = ch.c[c];
            const i64 zs = (i64)z0 + k + m.dz - m.first, ys = (i64)y + m.dy, xs = (i64)x + m.dx;
            Tin v = 0;
            if (m.src && (u64)zs < (u64)m.count && (u64)ys < (u64)m.ny && (u64)xs < (u64)m.nx)
                v = static_cast<const Tin*>(m.src)[(zs * m.ny + ys) * m.nx + xs];
            px.c[c] = (Tout)v;
        }
        out[i] = px;
    }
}

template <class Tin>
int composite_launch(hipStream_t s, const Channels& ch, int z0, int n, int ny, int nx, void* out, int out_dtype) {
    const dim3 grid(pixel_blocks((i64)n * ny * nx)), block(kThreads);
    switch (out_dtype) {
        case MI_RGB_U8: hipLaunchKernelGGL((composite_kernel<Tin, uint8_t>), grid, block, 0, s, ch, z0, n, ny, nx, static_cast<Rgb<uint8_t>*>(out)); break;
        case MI_RGB_U16: hipLaunchKernelGGL((composite_kernel<Tin, uint16_t>), grid, block, 0, s, ch, z0, n, ny, nx, static_cast<Rgb<uint16_t>*>(out)); break;
        case MI_RGB_U32: hipLaunchKernelGGL((composite_kernel<Tin, uint32_t>), grid, block, 0, s, ch, z0, n, ny, nx, static_cast<Rgb<uint32_t>*>(out)); break;
        default: hipLaunchKernelGGL((composite_kernel<Tin, float>), grid, block, 0, s, ch, z0, n, ny, nx, static_cast<Rgb<float>*>(out)); break;
    }
    return launch_check("composite_kernel");
}

}  // namespace
}  // namespace mi

using namespace mi;

extern "C" int mi_sobel2d_f32(int device, void* stream, const float* in, int ny, int nx, float* out) {
    MI_TRY(use_device(device));
    const void* planes[] = {in, out};
    MI_TRY(check_planes("mi_sobel2d_f32", planes, 2, ny, nx, 1));
    hipLaunchKernelGGL(sobel_kernel, dim3(pixel_blocks((i64)ny * nx)), dim3(kThreads), 0, as_stream(stream), in, ny, nx, out);
    return launch_check("sobel_kernel");
}

extern "C" int mi_ecc_prepare(int device, void* stream, const float* tmpl, const float* subj, int ny, int nx, float* t, float* s, float* gx,
                              float* gy) {
    MI_TRY(use_device(device));
    const void* planes[] = {tmpl, subj, t, s, gx, gy};
    MI_TRY(check_planes("mi_ecc_prepare", planes, 6, ny, nx, 3));
    hipStream_t st = as_stream(stream);
    const unsigned blocks = pixel_blocks((i64)ny * nx);
    hipLaunchKernelGGL(blur5_kernel, dim3(blocks, 2), dim3(kThreads), 0, st, tmpl, subj, ny, nx, t, s);
    MI_TRY(launch_check("blur5_kernel"));
    hipLaunchKernelGGL(gradient_kernel, dim3(blocks), dim3(kThreads), 0, st, (const float*)s, ny, nx, gx, gy);
    return launch_check("gradient_kernel");
}

extern "C" int mi_ecc_sums(int device, void* stream, const float* t, const float* s, const float* gx, const float* gy, int ny, int nx,
                           double tx, double ty, double* scratch, double* sums) {
    MI_TRY(use_device(device));
    const void* planes[] = {t, s, gx, gy};
    MI_TRY(check_planes("mi_ecc_sums", planes, 4, ny, nx, 3));
    MI_REQUIRE(scratch && sums && ((uintptr_t)scratch % 8) == 0 && ((uintptr_t)sums % 8) == 0, "mi_ecc_sums: scratch and sums must be 8-byte aligned");
    hipStream_t st = as_stream(stream);
    const int groups = sum_groups(ny, nx);
    hipLaunchKernelGGL(ecc_sums_kernel, dim3(groups), dim3(kThreads), 0, st, t, s, gx, gy, ny, nx, (const mi_ecc_state*)nullptr, tx, ty, scratch);
    MI_TRY(launch_check("ecc_sums_kernel"));
    hipLaunchKernelGGL(ecc_total_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, groups, sums);
    return launch_check("ecc_total_kernel");
}

extern "C" int mi_ecc_translation_run(int device, void* stream, const float* t, const float* s, const float* gx, const float* gy, int ny,
                                      int nx, double tx0, double ty0, int iterations, double eps, int batch, mi_ecc_state* state,
                                      double* scratch, mi_ecc_state* result) {
    MI_TRY(use_device(device));
    const void* planes[] = {t, s, gx, gy};
    MI_TRY(check_planes("mi_ecc_translation_run", planes, 4, ny, nx, 3));
    MI_REQUIRE(state && scratch && result, "mi_ecc_translation_run: null pointer");
    MI_REQUIRE(((uintptr_t)state % 8) == 0 && ((uintptr_t)scratch % 8) == 0, "mi_ecc_translation_run: state and scratch must be 8-byte aligned");
    MI_REQUIRE(iterations >= 0 && eps >= 0.0, "mi_ecc_translation_run: iterations=%d eps=%g", iterations, eps);
    hipStream_t st = as_stream(stream);
    if (batch <= 0) batch = MI_ECC_DEFAULT_BATCH;
    const int groups = sum_groups(ny, nx);
    hipLaunchKernelGGL(ecc_init_kernel, dim3(1), dim3(1), 0, st, state, tx0, ty0, eps, iterations);
    MI_TRY(launch_check("ecc_init_kernel"));
    for (int enqueued = 0;;) {
        // once `done` is set the rest of a batch returns at once: a batch costs at most `batch` pairs of empty launches
        for (int k = 0; k < batch && enqueued < iterations; ++k, ++enqueued) {
            hipLaunchKernelGGL(ecc_sums_kernel, dim3(groups), dim3(kThreads), 0, st, t, s, gx, gy, ny, nx, (const mi_ecc_state*)state, 0.0, 0.0, scratch);
            MI_TRY(launch_check("ecc_sums_kernel"));
            hipLaunchKernelGGL(ecc_step_kernel, dim3(1), dim3(64), 0, st, (const double*)scratch, groups, state, iterations, eps);
            MI_TRY(launch_check("ecc_step_kernel"));
        }
        MI_HIP(hipMemcpyAsync(result, state, sizeof(mi_ecc_state), hipMemcpyDeviceToHost, st));
        MI_HIP(hipStreamSynchronize(st));
        if (result->done) return MI_OK;
        MI_REQUIRE(enqueued < iterations, "mi_ecc_translation_run: the state is not done after %d iterations", iterations);
    }
}

extern "C" int mi_channel_composite(int device, void* stream, const mi_composite_channel* channels, int src_dtype, int z0, int n, int ny,
                                    int nx, void* out, int out_dtype) {
    MI_TRY(use_device(device));
    MI_REQUIRE(channels && out, "mi_channel_composite: null pointer");
    MI_REQUIRE(src_dtype == MI_RGB_U8 || src_dtype == MI_RGB_U16, "mi_channel_composite: src_dtype=%d, MI_RGB_U8 or MI_RGB_U16", src_dtype);
    MI_REQUIRE(out_dtype >= MI_RGB_U8 && out_dtype <= MI_RGB_F32, "mi_channel_composite: out_dtype=%d, MI_RGB_U8 .. MI_RGB_F32", out_dtype);
    MI_REQUIRE(z0 >= 0 && n >= 1 && ny >= 1 && nx >= 1, "mi_channel_composite: z0=%d n=%d ny=%d nx=%d", z0, n, ny, nx);
    const size_t out_bytes = out_dtype == MI_RGB_U8 ? 1 : out_dtype == MI_RGB_U16 ? 2 : 4;
    MI_REQUIRE(((uintptr_t)out % out_bytes) == 0, "mi_channel_composite: out must be aligned to its sample type");
    Channels ch;
    for (int c = 0; c < 3; ++c) {
        ch.c[c] = channels[c];
        const mi_composite_channel& m = ch.c[c];
        if (!m.src) continue;
        MI_REQUIRE(m.count >= 1 && m.first >= 0 && m.ny >= 1 && m.nx >= 1, "mi_channel_composite: channel %d: count=%d first=%d ny=%d nx=%d", c,
                   m.count, m.first, m.ny, m.nx);
        MI_REQUIRE(src_dtype == MI_RGB_U8 || ((uintptr_t)m.src % 2) == 0, "mi_channel_composite: u16 sources must be 2-byte aligned");
    }
    hipStream_t st = as_stream(stream);
    if (src_dtype == MI_RGB_U8) return composite_launch<uint8_t>(st, ch, z0, n, ny, nx, out, out_dtype);
    return composite_launch<uint16_t>(st, ch, z0, n, ny, nx, out, out_dtype);
}
