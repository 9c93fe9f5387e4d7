// In-place separable 3-D Gaussian (replaces gauss3d_gpu: LsDeconvolveMultiGPU/gauss3d_gpu.cu:81-204,209-311).
//
// Same arithmetic as the reference: taps exp(-0.5 i^2 / sigma^2) built on the host (double exp, float
// store, double sum), filtered X, then Y, then Z with the index clamped to the volume, fp32 accumulate
// in tap order, every 1-D result rounded to fp32.  Execution (the reference moves 32 B/voxel: three passes
// plus a copy): ONE pass of 8 B/voxel when the z kernel is short enough for an LDS ring of xy-filtered
// planes (k_gauss3d_fused: the RL loop's regularisation step, which also ping-pongs its buffers so that
// no copy back is needed), else TWO passes of 16 B/voxel in all: x and y fused in a kernel whose waves walk
// along y with an LDS ring of x-filtered rows, z a second walk with a per-lane ring landing back in
// `vol`.  Taps travel in the kernel argument block.
#include <utility>
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "conv3d_direct.h"
#include "mi_internal.h"
#include "mi_lsdeconv.h"

namespace mi {
namespace {

constexpr int kMaxTaps = 51;  // MAX_KERNEL_SIZE, gauss3d_gpu.cu:77
struct Taps {
    float w[kMaxTaps];
    int n;
};

// make_gaussian_kernel, gauss3d_gpu.cu:81-90
void make_taps(float sigma, int ksize, Taps& t) {
    int r = ksize / 2;
    double sum = 0.0;
    float s2 = sigma * sigma;
    for (int i = -r; i <= r; ++i) {
        t.w[i + r] = static_cast<float>(std::exp(-0.5 * (i * i) / s2));
        sum += t.w[i + r];
    }
    for (int i = 0; i < ksize; ++i) t.w[i] = static_cast<float>(t.w[i] / sum);
    t.n = ksize;
}

// Pass 1 (x and y fused): a wave owns 64 consecutive x of one z-plane and walks along y.  Per step it stages one
// clamped row segment (64 + 2 rx samples) in LDS, filters it along x (the result is rounded to fp32 exactly like the
// reference's separate x pass), pushes it into a per-lane ring of the last ky x-filtered rows and emits one y-filtered
// row.  Every input row is read once and every output row written once (plus ry halo rows per y-chunk).
constexpr int GXY_WAVES = 4;
constexpr int GXY_YCHUNK = 256;

// orders the LDS traffic of ONE wave for the compiler (the hardware executes a wave's DS operations in order)
__device__ __forceinline__ void wave_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

__global__ __launch_bounds__(64 * GXY_WAVES) void k_gauss_xy(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz,
                                                              Taps tx, Taps ty) {
    extern __shared__ float lds[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int rx = tx.n / 2, ry = ty.n / 2;
    const int seg = 64 + 2 * rx;
    float* rb = lds + wave * (seg + ty.n * 64);  // row buffer, then ring[ty.n][64]
    float* ring = rb + seg;
    const int x0 = blockIdx.x * 64;
    const int ya = blockIdx.y * GXY_YCHUNK, yb = min(ya + GXY_YCHUNK, ny);
    const int z = blockIdx.z * GXY_WAVES + wave;
    const bool zlive = z < nz;
    const float* plane = src + (size_t)(zlive ? z : 0) * ny * nx;
    float* oplane = dst + (size_t)(zlive ? z : 0) * ny * nx;
    int slot = 0;  // ring slot of walk position p
    // the rows of the walk are requested GXY_PF steps ahead (one row per step, waited for at once, left the pass at 2 TB/s)
    constexpr int GXY_PF = 4;
    const int xa = min(max(x0 - rx + lane, 0), nx - 1), xb = min(max(x0 - rx + lane + 64, 0), nx - 1);
    const bool has_b = lane + 64 < seg;
    float pa[GXY_PF], pb[GXY_PF];
    auto fetch = [&](int p, float& a, float& b) {
        const float* row = plane + (size_t)min(max(p, 0), ny - 1) * nx;
        a = row[xa];
        b = has_b ? row[xb] : 0.0f;
    };
#pragma unroll
    for (int u = 0; u < GXY_PF; ++u) fetch(ya - ry + u, pa[u], pb[u]);
    // output row yo is emitted at walk position yo + lead, when the ring holds rows yo - ry .. yo - ry + ty.n - 1: the reference's
    // window (offset s - klen / 2, gauss3d_gpu.cu:124-135); lead == ry for odd tap counts, ry - 1 for even ones
    const int lead = ty.n - 1 - ry;
    for (int p = ya - ry; p < yb + lead; ++p) {
        // stage the clamped row segment: sample i is x = x0 - rx + i
        rb[lane] = pa[0];
        if (has_b) rb[lane + 64] = pb[0];
#pragma unroll
        for (int u = 0; u + 1 < GXY_PF; ++u) { pa[u] = pa[u + 1]; pb[u] = pb[u + 1]; }
        fetch(p + GXY_PF, pa[GXY_PF - 1], pb[GXY_PF - 1]);
        wave_fence();  // (the row buffer and the ring belong to this wave alone: DS operations of a wave execute in order)
        float xf = 0.0f;
        for (int s = 0; s < tx.n; ++s) xf = fmaf(rb[lane + s], tx.w[s], xf);
        ring[slot * 64 + lane] = xf;  // private column of this lane: no barrier needed for the ring
        const int yo = p - lead;      // output row whose window [yo - ry, yo - ry + ty.n - 1] is now complete
        if (yo >= ya) {
            float acc = 0.0f;
            int rs = slot + 1;  // slot of walk position yo - ry = p - ty.n + 1  (the oldest of the ty.n slots, wrapping)
            if (rs >= ty.n) rs -= ty.n;
            for (int s = 0; s < ty.n; ++s) {
                acc = fmaf(ring[rs * 64 + lane], ty.w[s], acc);
                if (++rs >= ty.n) rs = 0;
            }
            if (zlive && x0 + lane < nx) oplane[(size_t)yo * nx + x0 + lane] = acc;
        }
        if (++slot >= ty.n) slot = 0;
        wave_fence();  // the row buffer is rewritten in the next step
    }
}

// Pass 2 (z): a lane owns one (x, y) column and walks along z with a private LDS ring of the last kz samples.
constexpr int GZW_U = 8;  // output rows / planes per register-window chunk (k_gauss_xy_win, k_gauss_z_win)
// x then y filter with compile-time tap counts (equal in x and y: the usual case): a wave owns 64 columns of one z plane and
// walks its rows; a row is staged in the wave's LDS segment and x-filtered with N fixed-offset reads, the x-filtered rows of the
// y window live in REGISTERS (chunks of GZW_U output rows, as in k_gauss_z_win).  k_gauss_xy spent ~120 instructions per output
// on ring indices and LDS addresses (9.3 ms for 13 x 13 taps on a 2048 x 2048 x 512 block).  Each 1-D result is rounded to fp32
// like the reference's separate passes, taps in the same order.
template <int N>
__global__ __launch_bounds__(64 * GXY_WAVES) void k_gauss_xy_win(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz,
                                                                  Taps tx, Taps ty) {
    constexpr int R = N / 2, U = GZW_U, W = U + 2 * R, SEG = 64 + 2 * R, PF = 16;
    __shared__ float rbs[GXY_WAVES][SEG];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    float* rb = rbs[wave];
    const int x0 = blockIdx.x * 64;
    const int ya = blockIdx.y * GXY_YCHUNK, yb = min(ya + GXY_YCHUNK, ny);
    const int z = blockIdx.z * GXY_WAVES + wave;
    if (z >= nz) return;  // (no work-group barrier below: a wave may leave alone)
    const float* plane = src + (size_t)z * ny * nx;
    float* oplane = dst + (size_t)z * ny * nx;
    const int xa = min(max(x0 - R + lane, 0), nx - 1), xb = min(max(x0 - R + lane + 64, 0), nx - 1);
    const bool has_b = lane + 64 < SEG;
    float pa[PF], pb[PF];
    auto fetch = [&](int p, float& a, float& b) {
        const float* row = plane + (size_t)min(max(p, 0), ny - 1) * nx;
        a = row[xa];
        b = has_b ? row[xb] : 0.0f;
    };
    int pn = ya - R;  // next row to request
#pragma unroll
    for (int u = 0; u < PF; ++u) fetch(pn++, pa[u], pb[u]);
    // x-filtered value of the next row of the walk (rows arrive in order)
    auto next_xf = [&]() {
        rb[lane] = pa[0];
        if (has_b) rb[lane + 64] = pb[0];
#pragma unroll
        for (int u = 0; u + 1 < PF; ++u) { pa[u] = pa[u + 1]; pb[u] = pb[u + 1]; }
        fetch(pn++, pa[PF - 1], pb[PF - 1]);
        wave_fence();
        float xf = 0.0f;
#pragma unroll
        for (int s = 0; s < N; ++s) xf = fmaf(rb[lane + s], tx.w[s], xf);
        wave_fence();  // the segment is rewritten by the next call
        return xf;
    };
    float win[W];
#pragma unroll
    for (int i = 0; i < W - U; ++i) win[i] = next_xf();  // rows ya - R .. ya + R - 1
    const bool xlive = x0 + lane < nx;
    for (int y0 = ya; y0 < yb; y0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) win[W - U + u] = next_xf();  // rows y0 + R .. y0 + U - 1 + R
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.0f;
#pragma unroll
            for (int s = 0; s < N; ++s) acc = fmaf(win[u + s], ty.w[s], acc);
            if (xlive && y0 + u < yb) oplane[(size_t)(y0 + u) * nx + x0 + lane] = acc;
        }
#pragma unroll
        for (int i = 0; i < W - U; ++i) win[i] = win[i + U];
    }
}

constexpr int GZ_ZCHUNK = 512;
// z filter with the window of a column in REGISTERS (tap counts known at compile time): a lane walks its column in chunks of
// GZW_U outputs, keeps the GZW_U + N - 1 inputs they need in registers and requests the next chunk's GZW_U new planes before it
// reduces the current chunk -- N fused multiply-adds, one load and one store per output instead of N LDS reads with a wrapping
// ring index (k_gauss_z: 7.7 ms for 25 taps on a 2048 x 2048 x 512 block).  Same summation order as k_gauss_z.
template <int N>
__global__ __launch_bounds__(256) void k_gauss_z_win(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz, int zchunk,
                                                      Taps tz) {
    constexpr int R = N / 2, U = GZW_U, W = U + 2 * R;
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= nx) return;
    const int za = blockIdx.z * zchunk, zb = min(za + zchunk, nz);
    const size_t col = (size_t)y * nx + x, pstride = (size_t)ny * nx;
    auto fetch = [&](int z) { return src[col + (size_t)min(max(z, 0), nz - 1) * pstride]; };  // replicate rule (gauss3d_gpu.cu:124-137)
    float win[W], nxt[U];
#pragma unroll
    for (int i = 0; i < W; ++i) win[i] = fetch(za - R + i);
    for (int z0 = za; z0 < zb; z0 += U) {
#pragma unroll
        for (int u = 0; u < U; ++u) nxt[u] = fetch(z0 + U + R + u);
#pragma unroll
        for (int u = 0; u < U; ++u) {
            float acc = 0.0f;
#pragma unroll
            for (int s = 0; s < N; ++s) acc = fmaf(win[u + s], tz.w[s], acc);
            if (z0 + u < zb) dst[col + (size_t)(z0 + u) * pstride] = acc;
        }
#pragma unroll
        for (int i = 0; i < W - U; ++i) win[i] = win[i + U];
#pragma unroll
        for (int u = 0; u < U; ++u) win[W - U + u] = nxt[u];
    }
}

__global__ __launch_bounds__(256) void k_gauss_z(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz, Taps tz) {
    extern __shared__ float lds[];
    const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
    if (x >= nx) return;
    const int rz = tz.n / 2;
    const int za = blockIdx.z * GZ_ZCHUNK, zb = min(za + GZ_ZCHUNK, nz);
    const size_t col = (size_t)y * nx + x, pstride = (size_t)ny * nx;
    float* ring = lds + threadIdx.x;  // ring[slot * 256]
    int slot = 0;
    constexpr int PF = 8;  // planes requested ahead of the walk (one load per step left the pass latency-bound at 2 TB/s)
    float in[PF];
    const int lead = tz.n - 1 - rz;  // as in k_gauss_xy: rz for odd tap counts, rz - 1 for even ones
    const int p_end = zb + lead;
    auto fetch = [&](int p) { return src[col + (size_t)min(max(p, 0), nz - 1) * pstride]; };
#pragma unroll
    for (int u = 0; u < PF; ++u) in[u] = fetch(za - rz + u);  // (clamped: harmless beyond the end)
    for (int p0 = za - rz; p0 < p_end; p0 += PF) {
#pragma unroll
        for (int u = 0; u < PF; ++u) {
            const int p = p0 + u;
            if (p >= p_end) break;
            ring[slot * 256] = in[u];
            in[u] = fetch(p + PF);
            const int zo = p - lead;
            if (zo >= za) {
                float acc = 0.0f;
                int rs = slot + 1;
                if (rs >= tz.n) rs -= tz.n;
                for (int s = 0; s < tz.n; ++s) {
                    acc = fmaf(ring[rs * 256], tz.w[s], acc);
                    if (++rs >= tz.n) rs = 0;
                }
                dst[col + (size_t)zo * pstride] = acc;
            }
            if (++slot >= tz.n) slot = 0;
        }
    }
}

// Single pass (x, y and z fused): 8 B/voxel.  A work-group owns a 64 x 16 (x, y) tile and marches along z.  Per plane it stages
// the clamped (16 + 2 ry) x (64 + halo) input patch with 16-byte loads, filters it along x, then along y (every 1-D result
// rounded to fp32, like the reference's separate passes), pushes the 64 x 16 xy-filtered plane into an LDS ring of the last kz
// planes and emits one z-filtered plane with 16-byte stores.  A thread owns four neighbouring x of one row from the y filter
// on (its ring entries are private: no barrier between the y and z filters).  Used when the ring fits (kz <= 12 or so: the
// sigma = 0.5 regularisation step of the RL loop, 5 taps per axis); larger z kernels take the two-pass kernels above.
constexpr int GF_NPRE = 3;
template <int GF_TX, int GF_TY>
__global__ __launch_bounds__((GF_TX / 4) * GF_TY) void k_gauss3d_fused(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz,
                                                              int zchunk, Taps tx, Taps ty, Taps tz) {
    constexpr int GF_XQ = GF_TX / 4, GF_THREADS = GF_XQ * GF_TY;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int rx = tx.n / 2, ry = ty.n / 2, rz = tz.n / 2;
    const int cq = (rx + 3) / 4;              // x halo in float4 units per side
    const int segq = GF_TX / 4 + 2 * cq;      // float4 per staged row
    const int seg = 4 * segq, rows_in = GF_TY + 2 * ry;
    float* in = lds;                          // [rows_in][seg]
    float* xf = in + rows_in * seg;           // [rows_in][64]
    float* ring = xf + rows_in * GF_TX;       // [tz.n][16][64]
    const int tid = threadIdx.x, xq = tid % GF_XQ, rsub = tid / GF_XQ;
    // XCD-aware tile order: work-groups are dealt round-robin over the 8 XCDs, so linear id L goes to XCD L % 8; giving every XCD
    // a contiguous range of tiles (x fastest, then y, then z chunk) keeps the x / y halos of neighbouring tiles in ONE L2
    const int gx = (nx + GF_TX - 1) / GF_TX, gy = (ny + GF_TY - 1) / GF_TY, gz = (nz + zchunk - 1) / zchunk;
    const int total = gx * gy * gz, per = (total + 7) / 8;
    const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (t >= total) return;
    const int bz = t / (gx * gy), by = (t - bz * gx * gy) / gx, bx = t - bz * gx * gy - by * gx;
    const int x0 = bx * GF_TX, y0 = by * GF_TY;
    const int za = bz * zchunk, zb = min(za + zchunk, nz);
    const int xoff = 4 * cq - rx;             // first tap of output x sits at staged column x + xoff
    int slot = 0;
    // the patch of plane p + 1 is requested into registers before plane p is filtered: without it every plane of the march paid a
    // full HBM round trip (7 ms instead of 3 for a 2048 x 2048 x 512 volume)
    float4 pre[GF_NPRE];
    auto fetch = [&](int p) {
        const float* plane = src + (size_t)min(max(p, 0), nz - 1) * ny * nx;
#pragma unroll
        for (int u = 0; u < GF_NPRE; ++u) {
            const int it = tid + u * GF_THREADS;
            if (it < rows_in * segq) {
                const int r = it / segq, q = it - r * segq;
                const float* row = plane + (size_t)min(max(y0 - ry + r, 0), ny - 1) * nx;
                const int x = x0 - 4 * cq + 4 * q;
                if (x >= 0 && x + 3 < nx) pre[u] = *reinterpret_cast<const float4*>(row + x);
                else pre[u] = make_float4(row[min(max(x, 0), nx - 1)], row[min(max(x + 1, 0), nx - 1)], row[min(max(x + 2, 0), nx - 1)],
                                          row[min(max(x + 3, 0), nx - 1)]);
            }
        }
    };
    fetch(za - rz);
    for (int p = za - rz; p < zb + rz; ++p) {
#pragma unroll
        for (int u = 0; u < GF_NPRE; ++u) {
            const int it = tid + u * GF_THREADS;
            if (it < rows_in * segq) {
                const int r = it / segq, q = it - r * segq;
                *reinterpret_cast<float4*>(in + r * seg + 4 * q) = pre[u];
            }
        }
        __syncthreads();
        if (p + 1 < zb + rz) fetch(p + 1);
        for (int it = tid; it < rows_in * GF_XQ; it += GF_THREADS) {   // x filter: 4 outputs from kx + 3 staged samples
            const int r = it / GF_XQ, q = it % GF_XQ;
            const float* a = in + r * seg + 4 * q + xoff;
            float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
            float v0 = a[0], v1 = a[1], v2 = a[2];
            for (int t = 0; t < tx.n; ++t) {
                const float v3 = a[t + 3], w = tx.w[t];
                o0 = fmaf(v0, w, o0);
                o1 = fmaf(v1, w, o1);
                o2 = fmaf(v2, w, o2);
                o3 = fmaf(v3, w, o3);
                v0 = v1; v1 = v2; v2 = v3;
            }
            *reinterpret_cast<float4*>(xf + r * GF_TX + 4 * q) = make_float4(o0, o1, o2, o3);
        }
        __syncthreads();
        {   // y filter of row rsub, columns 4 xq .. + 3 -> ring[slot]
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int t = 0; t < ty.n; ++t) {
                const float4 v = *reinterpret_cast<const float4*>(xf + (rsub + t) * GF_TX + 4 * xq);
                const float w = ty.w[t];
                acc.x = fmaf(v.x, w, acc.x); acc.y = fmaf(v.y, w, acc.y); acc.z = fmaf(v.z, w, acc.z); acc.w = fmaf(v.w, w, acc.w);
            }
            *reinterpret_cast<float4*>(ring + ((size_t)slot * GF_TY + rsub) * GF_TX + 4 * xq) = acc;
        }
        const int zo = p - rz;  // output plane whose window [zo - rz, zo + rz] is now complete
        if (zo >= za) {
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            int rs = slot + 1;
            if (rs >= tz.n) rs -= tz.n;
            for (int t = 0; t < tz.n; ++t) {
                const float4 v = *reinterpret_cast<const float4*>(ring + ((size_t)rs * GF_TY + rsub) * GF_TX + 4 * xq);
                const float w = tz.w[t];
                acc.x = fmaf(v.x, w, acc.x); acc.y = fmaf(v.y, w, acc.y); acc.z = fmaf(v.z, w, acc.z); acc.w = fmaf(v.w, w, acc.w);
                if (++rs >= tz.n) rs = 0;
            }
            const int y = y0 + rsub, x = x0 + 4 * xq;
            if (y < ny && x < nx) *reinterpret_cast<float4*>(dst + ((size_t)zo * ny + y) * nx + x) = acc;
        }
        if (++slot >= tz.n) slot = 0;
        // (the next plane's staging overwrites `in`, last read before the second barrier above; `xf` is rewritten only behind
        // the next first barrier, which every thread reaches after its y filter)
    }
}

// The single pass, round 4 (k_gauss3d_wave).  A work-group owns a 64 x 32 (x, y) tile and marches along z; its four waves SHARE the
// staged input patch ((32 + 2 ry) rows: every input row is fetched 1.125 x 1.125 times -- with a patch per wave of 8 rows it was
// 1.5 x 1.125, PMC: 17.2 GB fetched for an 8.6-GB volume, and the pass ran at the HBM rate of THAT traffic) and nothing else: a wave
// filters the 8 + 2 ry rows it needs along x into its own slice of LDS, then along y in the lane that owns four neighbouring x of
// rows r and r + 4, and the z window -- the last KZ xy-filtered values of those 8 voxels -- never leaves the lane's registers (no
// LDS ring: k_gauss3d_fused writes a float4 and reads KZ per plane and lane).  ONE work-group barrier per plane, a whole plane away
// from where its data is needed: the patch is double-buffered, plane p + 2 is requested into registers while plane p is filtered,
// written to the other buffer one step later, used one step after that.
// Filters of the RL loop's regularisation step: kx, ky <= 7, kz = KZ in {3, 5, 7}; everything else takes the kernels above.
constexpr int GW_ROWS = 8, GW_MAXR = 3, GW_WGROWS = 32, GW_RIN = GW_WGROWS + 2 * GW_MAXR, GW_NPRE = 3;
// WX: the tile is 64 WX columns wide (WX waves side by side on each group of 8 rows, 256 WX threads): the x halo of a tile costs two
// 128-byte lines per row whatever its width -- 2 on 2 lines of payload for 64 columns, 2 on 4 for 128 (C3 volume: 4.2 -> 3.9 ms;
// 256 columns with 1024 threads: 4.0)
constexpr int GW_XF = (GW_ROWS + 2 * GW_MAXR) * 64;  // a wave's x-filtered rows
template <int KZ, int WX>
__global__ __launch_bounds__(256 * WX) void k_gauss3d_wave(const float* __restrict__ src, float* __restrict__ dst, int nx, int ny, int nz, int zchunk,
                                                       Taps tx, Taps ty, Taps tz) {
    constexpr int GW_TX = 64 * WX, GW_SEG = GW_TX + 8, NT = 256 * WX;
    __shared__ __attribute__((aligned(16))) float in2[2][GW_RIN * GW_SEG];   // the staged patch of two planes
    __shared__ __attribute__((aligned(16))) float xf_all[4 * WX * GW_XF];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int wx = wave % WX, wy = wave / WX;   // the wave's 64 columns and its 8 rows inside the tile
    float* xf = xf_all + wave * GW_XF;             // [rows of the wave][64]: after the x filter
    const int rx = tx.n / 2, ry = ty.n / 2, rows_in = GW_WGROWS + 2 * ry, rows_w = GW_ROWS + 2 * ry;
    constexpr int rz = KZ / 2, segq = GW_SEG / 4;
    // tiles as in k_gauss3d_fused: contiguous tile ranges per XCD
    const int gx = (nx + GW_TX - 1) / GW_TX, gy = (ny + GW_WGROWS - 1) / GW_WGROWS, gz = (nz + zchunk - 1) / zchunk;
    const int total = gx * gy * gz, per = (total + 7) / 8;
    const int t = (int)(blockIdx.x & 7) * per + (int)(blockIdx.x >> 3);
    if (t >= total) return;
    const int bz = t / (gx * gy), by = (t - bz * gx * gy) / gx, bx = t - bz * gx * gy - by * gx;
    const int x0 = bx * GW_TX, y0 = by * GW_WGROWS;
    const int za = bz * zchunk, zb = min(za + zchunk, nz);
    const int xoff = 4 - rx;                       // first tap of output x sits at staged column x + xoff
    const int xq = lane & 15, rs = lane >> 4;      // y / z filters: columns 4 xq .. + 3 of rows rs and rs + 4 of the wave's 8
    // a staged float4 lies wholly inside a row or wholly outside it (x0 and nx are multiples of 4): outside, it is the row's first
    // / last sample four times (replicate rule) -- the nearest inside float4 is loaded and one of its ends splatted
    float4 pre[GW_NPRE];
    int poff[GW_NPRE], pedge[GW_NPRE];
#pragma unroll
    for (int u = 0; u < GW_NPRE; ++u) {
        const int it = min(tid + NT * u, rows_in * segq - 1);   // (threads past the patch repeat its last piece: no predicated load)
        const int r = it / segq, q = it - r * segq, x = x0 - 4 + 4 * q;
        poff[u] = min(max(y0 - ry + r, 0), ny - 1) * nx + min(max(x, 0), nx - 4);
        pedge[u] = x < 0 ? -1 : (x >= nx ? 1 : 0);
    }
    auto fetch = [&](int p) {
        const float* plane = src + (size_t)min(max(p, 0), nz - 1) * ny * nx;
#pragma unroll
        for (int u = 0; u < GW_NPRE; ++u) {
            float4 v = *reinterpret_cast<const float4*>(plane + poff[u]);
            if (pedge[u] < 0) v = make_float4(v.x, v.x, v.x, v.x);
            if (pedge[u] > 0) v = make_float4(v.w, v.w, v.w, v.w);
            pre[u] = v;
        }
    };
    auto stage = [&](float* buf) {
#pragma unroll
        for (int u = 0; u < GW_NPRE; ++u) {
            const int it = tid + NT * u;
            if (it < rows_in * segq) {
                const int r = it / segq, q = it - r * segq;
                *reinterpret_cast<float4*>(buf + r * GW_SEG + 4 * q) = pre[u];
            }
        }
    };
    float4 win[KZ][2];  // the z window of the lane's 8 voxels, oldest first
#pragma unroll
    for (int i = 0; i < KZ; ++i) win[i][0] = win[i][1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const int p0 = za - rz, p1 = zb + rz;
    fetch(p0);
    stage(in2[0]);
    fetch(p0 + 1);
    __syncthreads();
    for (int p = p0; p < p1; ++p) {
        const float* in = in2[(p - p0) & 1] + wy * GW_ROWS * GW_SEG + 64 * wx;   // the wave's rows and columns of plane p
        stage(in2[(p - p0 + 1) & 1]);                                      // plane p + 1 (requested one step ago)
        fetch(p + 2);                                                      // (clamped planes past the chunk: harmless)
        for (int it = lane; it < rows_w * 16; it += 64) {   // x filter: 4 outputs from kx + 3 staged samples
            const int r = it >> 4, q = it & 15;
            const float* a = in + r * GW_SEG + 4 * q + xoff;
            float o0 = 0.0f, o1 = 0.0f, o2 = 0.0f, o3 = 0.0f;
            float v0 = a[0], v1 = a[1], v2 = a[2];
            for (int k = 0; k < tx.n; ++k) {
                const float v3 = a[k + 3], w = tx.w[k];
                o0 = fmaf(v0, w, o0);
                o1 = fmaf(v1, w, o1);
                o2 = fmaf(v2, w, o2);
                o3 = fmaf(v3, w, o3);
                v0 = v1; v1 = v2; v2 = v3;
            }
            *reinterpret_cast<float4*>(xf + r * 64 + 4 * q) = make_float4(o0, o1, o2, o3);
        }
        wave_fence();
#pragma unroll
        for (int i = 0; i + 1 < KZ; ++i) { win[i][0] = win[i + 1][0]; win[i][1] = win[i + 1][1]; }
#pragma unroll
        for (int h = 0; h < 2; ++h) {   // y filter of rows rs and rs + 4
            float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            for (int k = 0; k < ty.n; ++k) {
                const float4 v = *reinterpret_cast<const float4*>(xf + (rs + 4 * h + k) * 64 + 4 * xq);
                const float w = ty.w[k];
                acc.x = fmaf(v.x, w, acc.x); acc.y = fmaf(v.y, w, acc.y); acc.z = fmaf(v.z, w, acc.z); acc.w = fmaf(v.w, w, acc.w);
            }
            win[KZ - 1][h] = acc;
        }
        const int zo = p - rz;  // output plane whose window [zo - rz, zo + rz] is now complete
        if (zo >= za) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                float4 acc = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int k = 0; k < KZ; ++k) {
                    const float4 v = win[k][h];
                    const float w = tz.w[k];
                    acc.x = fmaf(v.x, w, acc.x); acc.y = fmaf(v.y, w, acc.y); acc.z = fmaf(v.z, w, acc.z); acc.w = fmaf(v.w, w, acc.w);
                }
                const int y = y0 + wy * GW_ROWS + rs + 4 * h, x = x0 + 64 * wx + 4 * xq;
                if (y < ny && x < nx) *reinterpret_cast<float4*>(dst + ((size_t)zo * ny + y) * nx + x) = acc;
            }
        }
        __syncthreads();   // plane p + 1 is staged for everybody; nobody reads plane p's buffer any more (it is written next step)
    }
}

#ifndef MI_GAUSS_FUSED_LDS
#define MI_GAUSS_FUSED_LDS (64 * 1024)
#endif
constexpr size_t kFusedLdsMax = MI_GAUSS_FUSED_LDS;
// tile of the single-pass kernel: 64 x 16 (x, y) by default; MI_GAUSS_TILE=<tx>x<ty> picks another built one (measurements)
void fused_tile(int* tx, int* ty) {
    // (a function-local static with an initialiser: set once, under the language's own lock -- worker threads of one process call
    // this concurrently, and two lazily assigned ints could be seen half-set)
    static const std::pair<int, int> tile = [] {
        int a = 64, b = 16;
        if (const char* e = MI_PROBE_ENV("MI_GAUSS_TILE")) {
            int u = 0, v = 0;
            if (sscanf(e, "%dx%d", &u, &v) == 2 && ((u == 64 && (v == 16 || v == 32)) || (u == 128 && (v == 8 || v == 16)))) { a = u; b = v; }
        }
        return std::make_pair(a, b);
    }();
    *tx = tile.first;
    *ty = tile.second;
}
size_t fused_lds_bytes(const int* k) {
    int GF_TX, GF_TY;
    fused_tile(&GF_TX, &GF_TY);
    const int cq = (k[0] / 2 + 3) / 4, seg = 4 * (GF_TX / 4 + 2 * cq), rows_in = GF_TY + 2 * (k[1] / 2);
    return sizeof(float) * ((size_t)rows_in * seg + (size_t)rows_in * GF_TX + (size_t)k[2] * GF_TY * GF_TX);
}

int resolve_taps(const float* sigma, const int* ksize, int* k, Taps& tx, Taps& ty, Taps& tz) {
    for (int a = 0; a < 3; ++a) {
        MI_REQUIRE(sigma[a] > 0.0f, "gauss3d_gpu: sigma must be positive");
        k[a] = ksize ? ksize[a] : 2 * (int)std::ceil(3.0 * (double)sigma[a]) + 1;  // gauss3d_gpu.cu:244-261
        MI_REQUIRE(k[a] >= 1 && k[a] <= kMaxTaps, "gauss3d_gpu: Kernel size exceeds MAX_KERNEL_SIZE (%d)", kMaxTaps);
    }
    make_taps(sigma[0], k[0], tx);
    make_taps(sigma[1], k[1], ty);
    make_taps(sigma[2], k[2], tz);
    return MI_OK;
}

}  // namespace

// whether the single-pass kernel takes this filter on this volume (odd kernel sizes, rows of whole float4, the ring in 64 KB)
bool gauss3d_fuses(int nx, const int* k) {
    int GF_TX, GF_TY;
    fused_tile(&GF_TX, &GF_TY);
    const int cq = (k[0] / 2 + 3) / 4, patch = (GF_TY + 2 * (k[1] / 2)) * (GF_TX / 4 + 2 * cq);  // float4 of a staged patch
    return (nx % 4) == 0 && (k[0] & 1) && (k[1] & 1) && (k[2] & 1) && fused_lds_bytes(k) <= kFusedLdsMax && patch <= GF_NPRE * (GF_TX / 4) * GF_TY;
}

// The kernels that filter an nx x ny x nz volume with tap counts k: the ONE place where the route is decided (gauss3d_to launches
// from this, mi_gauss3d_route reports it, so a test can assert the route it means to cover).  Pure host arithmetic.
constexpr bool gauss_win_built(int n) { return n >= 3 && n <= 25 && (n & 1); }  // k_gauss_xy_win<N> / k_gauss_z_win<N> exist for these N
struct GaussRoute {
    int kind;      // MI_GAUSS_ROUTE_WAVE, _FUSED or _TWO_PASS
    int wx;        // wave: tiles of 64 wx columns
    bool xy_win;   // two-pass: k_gauss_xy_win (registers) instead of the k_gauss_xy ring
    bool z_win;    // two-pass: k_gauss_z_win instead of the k_gauss_z ring
};
enum { MI_GAUSS_ROUTE_WAVE = 1, MI_GAUSS_ROUTE_FUSED = 2, MI_GAUSS_ROUTE_TWO_PASS = 3 };
GaussRoute gauss3d_route(int nx, int ny, int nz, const int* k) {
    (void)nz;
    GaussRoute r{MI_GAUSS_ROUTE_TWO_PASS, 1, false, false};
    if (gauss3d_fuses(nx, k)) {
        // the filters of the RL loop's regularisation step (patch offsets inside a plane are 32-bit)
        const bool wave = k[0] <= 2 * GW_MAXR + 1 && k[1] <= 2 * GW_MAXR + 1 && (k[2] == 3 || k[2] == 5 || k[2] == 7) &&
                          (size_t)ny * nx < ((size_t)1 << 31);
        r.kind = wave ? MI_GAUSS_ROUTE_WAVE : MI_GAUSS_ROUTE_FUSED;
        if (wave) r.wx = nx >= 512 ? 2 : 1;   // tiles of 128 columns where a row has enough of them
        return r;
    }
    r.xy_win = k[0] == k[1] && gauss_win_built(k[0]);   // the usual odd sizes, equal in x and y; others take the LDS ring
    r.z_win = gauss_win_built(k[2]);
    return r;
}
// the code of mi_gauss3d_route (include/mi_lsdeconv.h)
int gauss3d_route_code(const GaussRoute& r) {
    if (r.kind == MI_GAUSS_ROUTE_WAVE) return r.wx == 2 ? 2 : 1;
    if (r.kind == MI_GAUSS_ROUTE_FUSED) return 3;
    return 4 + (r.xy_win ? 1 : 0) + (r.z_win ? 2 : 0);
}

// out-of-place: dst = G(src), one pass when gauss3d_fuses(); *fused tells the caller which route ran (the two-pass route needs
// dst as its intermediate and leaves the result in SRC: the reference's in-place contract)
int gauss3d_to(hipStream_t s, float* src, float* dst, int nx, int ny, int nz, const float* sigma, const int* ksize, bool* fused) {
    MI_REQUIRE(src && dst && src != dst, "gauss3d_gpu: null or aliased buffers");
    MI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "gauss3d_gpu: Input must be 3D.");
    MI_REQUIRE(((uintptr_t)src % 16) == 0 && ((uintptr_t)dst % 16) == 0, "gauss3d_gpu: buffers must be 16-byte aligned");
    int k[3];
    Taps tx, ty, tz;
    MI_TRY(resolve_taps(sigma, ksize, k, tx, ty, tz));
    GaussRoute route = gauss3d_route(nx, ny, nz, k);
    *fused = route.kind != MI_GAUSS_ROUTE_TWO_PASS;
#ifdef MI_PROBES
    // (probe builds) the filter as a separable convolution with the replicate rule (sep3d.hip: k_sep3d_acc).  Bit-identical to the
    // kernels below; measured on a C3-sized volume incl. the copy back (profiles/gauss_time.py): 5 taps 8.6 against 8.4 ms,
    // 13 x 13 x 25 taps 16.6 against 7.8 ms for the two passes below -- so the Gaussian keeps its own kernels.
    if (MI_PROBE_ENV("MI_GAUSS_VIA_SEP")) {
        const int offs[3] = {k[0] / 2, k[1] / 2, k[2] / 2}, bnd[3] = {MI_BOUNDARY_REPLICATE, MI_BOUNDARY_REPLICATE, MI_BOUNDARY_REPLICATE};
        if ((k[0] & 1) && (k[1] & 1) && (k[2] & 1) && sep3d_fits(nx, k, offs)) {
            SepTaps t[3];
            const Taps* g3[3] = {&tx, &ty, &tz};
            for (int a = 0; a < 3; ++a) {
                t[a].n = k[a];
                for (int i = 0; i < k[a]; ++i) t[a].w[i] = g3[a]->w[i];
            }
            *fused = true;
            return sep3d_launch(s, src, dst, nx, ny, nz, t, offs, bnd, EPI_NONE, ConvEpilogue{});
        }
    }
#endif
    static const bool no_wave = MI_PROBE_ENV("MI_GAUSS_NO_WAVE") != nullptr;  // (probe builds: A/B against the work-group kernel)
    if (no_wave && route.kind == MI_GAUSS_ROUTE_WAVE) route.kind = MI_GAUSS_ROUTE_FUSED;
    if (route.kind == MI_GAUSS_ROUTE_WAVE) {
        const int zchunk = 128;
        int wx = route.wx;
        if (const char* e = MI_PROBE_ENV("MI_GAUSS_WX")) wx = atoi(e) == 2 ? 2 : 1;
        const int total = ((nx + 64 * wx - 1) / (64 * wx)) * ((ny + 31) / 32) * ((nz + zchunk - 1) / zchunk);
        const dim3 grid((total + 7) / 8 * 8), block(256 * wx);
#define MI_GW(KZV, WXV) hipLaunchKernelGGL((k_gauss3d_wave<KZV, WXV>), grid, block, 0, s, src, dst, nx, ny, nz, zchunk, tx, ty, tz)
        if (wx == 2) {
            if (k[2] == 3) MI_GW(3, 2); else if (k[2] == 5) MI_GW(5, 2); else MI_GW(7, 2);
        } else {
            if (k[2] == 3) MI_GW(3, 1); else if (k[2] == 5) MI_GW(5, 1); else MI_GW(7, 1);
        }
#undef MI_GW
        return launch_check("k_gauss3d_wave");
    }
    if (route.kind == MI_GAUSS_ROUTE_FUSED) {
        int GF_TX, GF_TY;
        fused_tile(&GF_TX, &GF_TY);
        int zchunk = k[2] <= 7 ? 128 : 256;
        if (const char* e = MI_PROBE_ENV("MI_GAUSS_ZCHUNK")) zchunk = std::max(2 * k[2], atoi(e));
        const int total = ((nx + GF_TX - 1) / GF_TX) * ((ny + GF_TY - 1) / GF_TY) * ((nz + zchunk - 1) / zchunk);
        const size_t lds = fused_lds_bytes(k);
        const dim3 grid((total + 7) / 8 * 8), block((GF_TX / 4) * GF_TY);
#define MI_GF(TXV, TYV)                                                                                                                 \
    if (GF_TX == TXV && GF_TY == TYV) {                                                                                                 \
        if (lds > 64 * 1024)                                                                                                            \
            MI_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_gauss3d_fused<TXV, TYV>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        hipLaunchKernelGGL((k_gauss3d_fused<TXV, TYV>), grid, block, lds, s, src, dst, nx, ny, nz, zchunk, tx, ty, tz);                  \
        launched = true;                                                                                                                 \
    }
        bool launched = false;
        MI_GF(64, 16) MI_GF(64, 32) MI_GF(128, 8) MI_GF(128, 16)
#undef MI_GF
        if (!launched) return fail(MI_ERR_INVALID, "gauss3d_gpu: no single-pass kernel for a %d x %d tile", GF_TX, GF_TY);
        return launch_check("k_gauss3d_fused");
    }
    // pass 1: src -> dst (x then y, each rounded to fp32 like the reference's separate passes); pass 2: dst -> src (z)
    const dim3 gxy((nx + 63) / 64, (ny + GXY_YCHUNK - 1) / GXY_YCHUNK, (nz + GXY_WAVES - 1) / GXY_WAVES);
    if (route.xy_win) {
#define MI_GXY(N) case N: hipLaunchKernelGGL(k_gauss_xy_win<N>, gxy, dim3(64 * GXY_WAVES), 0, s, src, dst, nx, ny, nz, tx, ty); break;
        switch (k[0]) {  // every N of gauss_win_built()
            MI_GXY(3) MI_GXY(5) MI_GXY(7) MI_GXY(9) MI_GXY(11) MI_GXY(13) MI_GXY(15) MI_GXY(17) MI_GXY(19) MI_GXY(21) MI_GXY(23) MI_GXY(25)
            default: return fail(MI_ERR_INVALID, "gauss3d_gpu: no k_gauss_xy_win for %d taps", k[0]);
        }
#undef MI_GXY
        MI_TRY(launch_check("k_gauss_xy_win"));
    } else {
        const size_t lds_xy = sizeof(float) * GXY_WAVES * (size_t)(64 + 2 * (k[0] / 2) + k[1] * 64);
        hipLaunchKernelGGL(k_gauss_xy, gxy, dim3(64 * GXY_WAVES), lds_xy, s, src, dst, nx, ny, nz, tx, ty);
        MI_TRY(launch_check("k_gauss_xy"));
    }
    const dim3 gz((nx + 255) / 256, ny, (nz + GZ_ZCHUNK - 1) / GZ_ZCHUNK);
    if (route.z_win) {
#define MI_GZ(N) case N: hipLaunchKernelGGL(k_gauss_z_win<N>, gz, dim3(256), 0, s, dst, src, nx, ny, nz, GZ_ZCHUNK, tz); break;
        switch (k[2]) {  // every N of gauss_win_built()
            MI_GZ(3) MI_GZ(5) MI_GZ(7) MI_GZ(9) MI_GZ(11) MI_GZ(13) MI_GZ(15) MI_GZ(17) MI_GZ(19) MI_GZ(21) MI_GZ(23) MI_GZ(25)
            default: return fail(MI_ERR_INVALID, "gauss3d_gpu: no k_gauss_z_win for %d taps", k[2]);
        }
#undef MI_GZ
        return launch_check("k_gauss_z_win");
    }
    const size_t lds_z = sizeof(float) * 256 * (size_t)k[2];
    hipLaunchKernelGGL(k_gauss_z, gz, dim3(256), lds_z, s, dst, src, nx, ny, nz, tz);
    return launch_check("k_gauss_z");
}

int gauss3d_async(hipStream_t s, float* vol, float* work, int nx, int ny, int nz, const float* sigma, const int* ksize) {
    bool fused = false;
    MI_TRY(gauss3d_to(s, vol, work, nx, ny, nz, sigma, ksize, &fused));
    // the reference's contract is destructive in place (gauss3d_gpu.cu:289-293): the single-pass result goes back with one copy
    if (fused) MI_HIP(hipMemcpyAsync(vol, work, sizeof(float) * (size_t)nx * ny * nz, hipMemcpyDeviceToDevice, s));
    return MI_OK;
}

}  // namespace mi

extern "C" int mi_gauss3d_route(int nx, int ny, int nz, const float* sigma, const int* ksize) {
    MI_REQUIRE(sigma, "gauss3d_gpu: Usage: gauss3d_gpu(x, sigma [, kernel_size])");
    MI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "gauss3d_gpu: Input must be 3D.");
    int k[3];
    mi::Taps tx, ty, tz;
    MI_TRY(mi::resolve_taps(sigma, ksize, k, tx, ty, tz));
    return mi::gauss3d_route_code(mi::gauss3d_route(nx, ny, nz, k));
}

extern "C" int mi_gauss3d_inplace(int dev, void* stream, float* vol, float* work, int nx, int ny, int nz, const float* sigma,
                                  const int* ksize) {
    MI_TRY(mi::use_device(dev));
    MI_REQUIRE(sigma, "gauss3d_gpu: Usage: gauss3d_gpu(x, sigma [, kernel_size])");
    return mi::gauss3d_async(mi::as_stream(stream), vol, work, nx, ny, nz, sigma, ksize);
}
