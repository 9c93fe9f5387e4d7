// The halving pyramid of the TeraFly conversion (include/mi_pyramid.h): levels 1..n of one z-group of integer slices.
//
// One launch makes two levels.  A thread owns one voxel of the second level ("cell"): the up to 2 x 2 x s2 first-level voxels
// under it, each the mean / max of 2 x 2 x s1 input samples (s = 2 for a 3-D level, 1 for a 2-D one).  It reads those input
// samples once (4 consecutive columns of up to 4 rows and 4 planes: one 8-byte load per row for uint16 when the row length is a
// multiple of 4), stores the first-level voxels, and reduces them in registers to the second-level voxel.  Cells at an odd edge of
// the first level hold first-level voxels without a second-level one (the reference drops that last row / column / slice there).
// Deeper levels chain: the next launch reads the second level (1/64 or less of the input).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mi_internal.h"
#include "mi_pyramid.h"

namespace {

template <class T> struct Vec4;
template <> struct Vec4<uint16_t> { using type = uint2; };      // 4 x uint16 = 8 bytes
template <> struct Vec4<uint8_t> { using type = uint32_t; };    // 4 x uint8 = 4 bytes

template <class T>
__device__ __forceinline__ void load4(const T* p, uint32_t v[4]) {
    const typename Vec4<T>::type w = *reinterpret_cast<const typename Vec4<T>::type*>(p);
    if constexpr (sizeof(T) == 2) {
        v[0] = w.x & 0xffffu; v[1] = w.x >> 16; v[2] = w.y & 0xffffu; v[3] = w.y >> 16;
    } else {
        v[0] = w & 0xffu; v[1] = (w >> 8) & 0xffu; v[2] = (w >> 16) & 0xffu; v[3] = w >> 24;
    }
}

// combine: running mean-sum or max of samples (exact in uint32 for <= 8 x 65535)
template <bool MAX>
__device__ __forceinline__ uint32_t comb(uint32_t a, uint32_t b) { return MAX ? (a > b ? a : b) : a + b; }

template <bool MAX>
__device__ __forceinline__ uint32_t finish(uint32_t acc, int three_d) {
    if (MAX) return acc;
    return three_d ? (acc + 4u) >> 3 : (acc + 2u) >> 2;   // iim::round(sum / 8.0f), iim::round(sum / 4.0f)
}

// in: nz x ny x nx.  Level 1: x1 = nx/2, y1 = ny/2, z1 = nz/s1.  Level 2 (when out2 or has2): x1/2, y1/2, z1/s2.
// VEC: nx % 4 == 0 (every row start and column 4*cx is aligned to 4 samples).
template <class T, bool MAX, bool VEC>
__global__ void __launch_bounds__(256) halve2_kernel(const T* __restrict__ in, int nx, int ny, int nz, int s1, int s2, int has2,
                                                     T* __restrict__ out1, T* __restrict__ out2) {
    const int cx = blockIdx.x * 64 + threadIdx.x;
    const int cy = blockIdx.y * 4 + threadIdx.y;
    const int cz = blockIdx.z;
    const int x1 = nx >> 1, y1 = ny >> 1, z1 = nz / s1;
    if (2 * cx >= x1 || 2 * cy >= y1) return;
    const int64_t plane0 = (int64_t)nx * ny;
    const int64_t plane1 = (int64_t)x1 * y1;
    uint32_t acc2 = 0;
    int n1 = 0;   // first-level voxels under this cell
    for (int dz = 0; dz < s2; ++dz) {
        const int zz = cz * s2 + dz;
        if (zz >= z1) break;
        // level-1 accumulators of the 2 x 2 voxels (rows 2cy, 2cy+1; columns 2cx, 2cx+1) of plane zz
        uint32_t a[2][2] = {{0, 0}, {0, 0}};
        const bool row_ok[2] = {true, 2 * cy + 1 < y1};
        const bool col_ok[2] = {true, 2 * cx + 1 < x1};
        for (int pz = 0; pz < s1; ++pz) {
            const T* base = in + (int64_t)(zz * s1 + pz) * plane0 + (int64_t)(4 * cy) * nx + 4 * cx;
            for (int r = 0; r < 4; ++r) {
                if (!row_ok[r >> 1]) break;
                uint32_t v[4];
                const T* p = base + (int64_t)r * nx;
                if (VEC) {
                    load4<T>(p, v);
                } else {
                    v[0] = p[0];
                    v[1] = p[1];
                    v[2] = col_ok[1] ? (uint32_t)p[2] : 0u;
                    v[3] = col_ok[1] ? (uint32_t)p[3] : 0u;
                }
                uint32_t* row = a[r >> 1];
                // sample order of the reference's sum: (z,i,j), (z,i,j+1), (z,i+1,j), (z,i+1,j+1), then z+1 -- any order is exact
                if (pz == 0 && (r & 1) == 0) {
                    row[0] = comb<MAX>(v[0], v[1]);
                    row[1] = comb<MAX>(v[2], v[3]);
                } else {
                    row[0] = comb<MAX>(row[0], comb<MAX>(v[0], v[1]));
                    row[1] = comb<MAX>(row[1], comb<MAX>(v[2], v[3]));
                }
            }
        }
        for (int i = 0; i < 2; ++i) {
            if (!row_ok[i]) break;
            for (int j = 0; j < 2; ++j) {
                if (!col_ok[j]) break;
                const uint32_t v1 = finish<MAX>(a[i][j], s1 == 2);
                if (out1) out1[(int64_t)zz * plane1 + (int64_t)(2 * cy + i) * x1 + 2 * cx + j] = (T)v1;
                acc2 = n1 == 0 ? v1 : comb<MAX>(acc2, v1);
                ++n1;
            }
        }
    }
    if (!has2 || !out2) return;
    const int x2 = x1 >> 1, y2 = y1 >> 1, z2 = z1 / s2;
    if (cx < x2 && cy < y2 && cz < z2)
        out2[(int64_t)cz * x2 * y2 + (int64_t)cy * x2 + cx] = (T)finish<MAX>(acc2, s2 == 2);
}

template <class T, bool MAX>
int launch(hipStream_t st, const void* in, int nx, int ny, int nz, int s1, int s2, int has2, void* o1, void* o2) {
    const int x1 = nx >> 1, y1 = ny >> 1, z1 = nz / s1;
    if (x1 <= 0 || y1 <= 0 || z1 <= 0) return MI_OK;   // nothing at this level (the caller sizes the outputs accordingly)
    const int cxn = (x1 + 1) / 2, cyn = (y1 + 1) / 2, czn = has2 ? (z1 + s2 - 1) / s2 : z1;
    MI_REQUIRE(czn <= 65535, "mi_pyramid_slab: %d planes in one launch (at most 65535)", czn);
    MI_REQUIRE((cyn + 3) / 4 <= 65535, "mi_pyramid_slab: %d rows (at most 524280)", ny);
    const dim3 block(64, 4, 1), grid(mi::cdiv(cxn, 64), mi::cdiv(cyn, 4), czn);
    const T* src = static_cast<const T*>(in);
    T* d1 = static_cast<T*>(o1);
    T* d2 = static_cast<T*>(o2);
    const int s2e = has2 ? s2 : 1;
    if (nx % 4 == 0 && (reinterpret_cast<uintptr_t>(in) % (4 * sizeof(T))) == 0)
        hipLaunchKernelGGL((halve2_kernel<T, MAX, true>), grid, block, 0, st, src, nx, ny, nz, s1, s2e, has2, d1, d2);
    else
        hipLaunchKernelGGL((halve2_kernel<T, MAX, false>), grid, block, 0, st, src, nx, ny, nz, s1, s2e, has2, d1, d2);
    return mi::launch_check("halve2_kernel");
}

}  // namespace

extern "C" int mi_pyramid_slab(int dev, void* stream, const void* in, int bytes, int nx, int ny, int nz, int method, int n_levels,
                               const int* halve_d, void* const* out) {
    MI_REQUIRE(in && halve_d && out, "mi_pyramid_slab: null pointer");
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_pyramid_slab: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(method == MI_HALVE_MEAN || method == MI_HALVE_MAX, "mi_pyramid_slab: method %d (mean 0, max 1)", method);
    MI_REQUIRE(nx > 0 && ny > 0 && nz > 0, "mi_pyramid_slab: slab of %d x %d x %d", nx, ny, nz);
    MI_REQUIRE(n_levels >= 1 && n_levels <= 30, "mi_pyramid_slab: %d levels", n_levels);
    {
        int64_t lx = nx, ly = ny, lz = nz;
        for (int k = 0; k < n_levels; ++k) {
            MI_REQUIRE(halve_d[k] == 0 || halve_d[k] == 1, "mi_pyramid_slab: halve_d[%d] = %d (0 or 1)", k, halve_d[k]);
            lx >>= 1;
            ly >>= 1;
            lz = halve_d[k] ? lz / 2 : lz;
            const bool empty = lx * ly * lz == 0;   // an empty level is never written (nor any level below it)
            MI_REQUIRE(out[k] || empty || !(k % 2 == 1 && k + 1 < n_levels),
                       "mi_pyramid_slab: level %d feeds level %d and needs a buffer", k + 1, k + 2);
        }
    }
    MI_TRY(mi::use_device(dev));
    hipStream_t st = mi::as_stream(stream);
    const void* src = in;
    int x = nx, y = ny, z = nz;
    for (int k = 0; k < n_levels; k += 2) {
        const int s1 = halve_d[k] ? 2 : 1;
        const int has2 = k + 1 < n_levels;
        const int s2 = has2 && halve_d[k + 1] ? 2 : 1;
        void* o2 = has2 ? out[k + 1] : nullptr;
        if (bytes == 2)
            MI_TRY((method == MI_HALVE_MAX ? launch<uint16_t, true>(st, src, x, y, z, s1, s2, has2, out[k], o2)
                                           : launch<uint16_t, false>(st, src, x, y, z, s1, s2, has2, out[k], o2)));
        else
            MI_TRY((method == MI_HALVE_MAX ? launch<uint8_t, true>(st, src, x, y, z, s1, s2, has2, out[k], o2)
                                           : launch<uint8_t, false>(st, src, x, y, z, s1, s2, has2, out[k], o2)));
        // dims of the level the next launch starts from
        x >>= 1; y >>= 1; z /= s1;
        if (has2) { x >>= 1; y >>= 1; z /= s2; }
        src = o2;
        if (x < 2 || y < 2 || z < 1) {
            // the deeper levels are empty: nothing to launch (their buffers have no samples)
            break;
        }
    }
    return MI_OK;
}
