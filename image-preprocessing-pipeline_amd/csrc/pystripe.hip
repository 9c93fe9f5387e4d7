// pystripe tile preprocessing: the plan, a run over a chunk of tiles and the C ABI, with the kernels that need no wavelet (uniform
// tiles, flat field and down-sample, the filter-less path).  The stages and the unit of each: pystripe_internal.h.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "pystripe_internal.h"

namespace mi {
namespace ps {
namespace {

// is_uniform_2d (:107): varies[tile] |= any sample differs from the first.  VEC: 16-byte loads (the tile's bytes are a multiple of 16 and
// the batch is 16-byte aligned).
template <class T, bool VEC>
__global__ void __launch_bounds__(256) uniform_kernel(const T* in, i64 npix, int* varies) {
    const i64 tile = blockIdx.y;
    const T* p = in + tile * npix;
    const T first = p[0];
    bool d = false;
    const i64 t0 = (i64)blockIdx.x * blockDim.x + threadIdx.x, step = (i64)gridDim.x * blockDim.x;
    if (VEC) {
        constexpr int E = 16 / sizeof(T);
        const uint4* p4 = reinterpret_cast<const uint4*>(p);
        for (i64 i = t0; i < npix / E; i += step) {
            union { uint4 v; T e[E]; } u;
            u.v = p4[i];
#pragma unroll
            for (int q = 0; q < E; ++q) d |= (u.e[q] != first);
        }
    } else {
        for (i64 i = t0; i < npix; i += step) d |= (p[i] != first);
    }
    // one atomic per wave that saw a difference, and none once the flag is up (a stale read only costs a redundant atomic)
    if (__any(d) && (threadIdx.x & 63) == 0 && __atomic_load_n(&varies[tile], __ATOMIC_RELAXED) == 0) atomicOr(&varies[tile], 1);
}

template <class T>
int launch_uniform(hipStream_t st, const void* in, i64 npix, int cnt, int* varies) {
    const bool vec = (npix * sizeof(T)) % 16 == 0 && reinterpret_cast<uintptr_t>(in) % 16 == 0;
    const i64 items = vec ? npix * (i64)sizeof(T) / 16 : npix;
    const dim3 grid((unsigned)std::max<i64>(1, std::min<i64>((items + 256 * 4 - 1) / (256 * 4), 2048)), cnt);
    if (vec) hipLaunchKernelGGL((uniform_kernel<T, true>), grid, dim3(256), 0, st, static_cast<const T*>(in), npix, varies);
    else hipLaunchKernelGGL((uniform_kernel<T, false>), grid, dim3(256), 0, st, static_cast<const T*>(in), npix, varies);
    return launch_check("uniform_kernel");
}

// flat field and skimage's block_reduce (zero padding up to a multiple of the block) -> a float32 tile
__global__ void __launch_bounds__(256) pre_kernel(Src s, const float* flat, int by, int bx, int method, float* stage, int ny, int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= nx || y >= ny) return;
    double sum = 0.0;
    float mx = -INFINITY, mn = INFINITY;
    for (int dy = 0; dy < by; ++dy)
        for (int dx = 0; dx < bx; ++dx) {
            const int yy = y * by + dy, xx = x * bx + dx;
            float v = 0.f;
            if (yy < s.ny && xx < s.nx) {
                v = src_load(s, tile, yy, xx);
                if (flat) v = v / flat[(i64)yy * s.nx + xx];
            }
            sum += (double)v;
            mx = fmaxf(mx, v);
            mn = fminf(mn, v);
        }
    const float r = method == MI_PS_DOWN_MAX ? mx : method == MI_PS_DOWN_MIN ? mn : (float)(sum / (double)(by * bx));
    stage[tile * ((i64)ny * nx) + (i64)y * nx + x] = r;
}

// block_reduce with numpy.median: the by * bx <= N samples of a block (zeros beyond the tile, +inf up to N) are sorted in registers
// by a bitonic network, every index static; an even count gives the mean of the two middle values, taken in float64.
template <int N>
__global__ void __launch_bounds__(256) pre_median_kernel(Src s, const float* flat, int by, int bx, float* stage, int ny, int nx) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    const i64 tile = blockIdx.z;
    if (x >= nx || y >= ny) return;
    const int cnt = by * bx;
    float v[N];
    int dy = 0, dx = 0;
#pragma unroll
    for (int e = 0; e < N; ++e) {
        float t = INFINITY;
        if (e < cnt) {
            const int yy = y * by + dy, xx = x * bx + dx;
            t = 0.f;
            if (yy < s.ny && xx < s.nx) {
                t = src_load(s, tile, yy, xx);
                if (flat) t = t / flat[(i64)yy * s.nx + xx];
            }
            if (++dx == bx) { dx = 0; ++dy; }
        }
        v[e] = t;
    }
#pragma unroll
    for (int k = 2; k <= N; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) {
                const int l = i ^ j;
                if (l > i) {
                    const bool up = (i & k) == 0;
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
        }
    }
    const int k0 = (cnt - 1) / 2, k1 = cnt / 2;
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        if (i == k0) a = v[i];
        if (i == k1) b = v[i];
    }
    stage[tile * ((i64)ny * nx) + (i64)y * nx + x] = (float)(((double)a + (double)b) * 0.5);
}

template <int N>
int launch_pre_median(hipStream_t st, dim3 grid, const Src& s, const float* flat, int by, int bx, float* stage, int ny, int nx) {
    hipLaunchKernelGGL(pre_median_kernel<N>, grid, dim3(256), 0, st, s, flat, by, bx, stage, ny, nx);
    return launch_check("pre_median_kernel");
}

// no stripe filter: every sample straight to the sink
__global__ void __launch_bounds__(256) point_kernel(Src s, Sink k) {
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= k.nx || y >= k.ny) return;
    sink_store(k, blockIdx.z, y, x, src_load(s, blockIdx.z, y, x));
}

int notch_rise_point(double sigma, double rise) {   // :670
    return (int)(std::sqrt(-2.0 * sigma * sigma * std::log(1.0 - rise)) + 0.5) / 2 * 2;
}

int pad_size(int ny, int nx, double sigma) {   // calculate_pad_size :681
    if (sigma == 0) return 0;
    const double x = nx + 1.0, y = ny + 1.0, c = 5e14;
    const double s = std::sqrt(x * x - 2 * x * y + y * y + 4 * c);
    const double r = std::nearbyint((1.0 - std::exp((x + y - s) / (4 * sigma * sigma))) * 100.0) / 100.0 - 0.01;
    return notch_rise_point(sigma, std::min(r, 0.5));
}

int max_level(int n, int L) { return n >= L - 1 ? std::max((int)std::floor(std::log2((double)n / (L - 1))), 0) : 0; }   // pywt.dwt_max_level

// sizes, modes and the scratch layout: everything that needs no device.  taps: of the wavelet the generic kernels run; 0: db9
int derive(int ny_in, int nx_in, int in_dtype, const mi_pystripe_params& q, int taps, Plan& P) {
    if (taps) { P.L = taps; P.generic = true; }
    MI_REQUIRE(ny_in > 0 && nx_in > 0, "mi_pystripe: tile of %d x %d", ny_in, nx_in);
    MI_REQUIRE(in_dtype >= MI_PS_U8 && in_dtype <= MI_PS_F32, "mi_pystripe: in_dtype %d (0 uint8, 1 uint16, 2 float32)", in_dtype);
    MI_REQUIRE(q.out_dtype >= MI_PS_U8 && q.out_dtype <= MI_PS_F32, "mi_pystripe: out_dtype %d (0 uint8, 1 uint16, 2 float32)", q.out_dtype);
    MI_REQUIRE(q.sigma1 >= 0 && q.sigma2 >= 0, "mi_pystripe: sigma (%g, %g) is negative", q.sigma1, q.sigma2);
    P.filter = q.sigma1 > 0 || q.sigma2 > 0;
    MI_REQUIRE(!P.filter || (q.sigma1 > 0 && q.sigma2 > 0), "np_notch: sigma must be positive (sigma = (%g, %g))", q.sigma1, q.sigma2);
    MI_REQUIRE(q.padding_mode >= MI_PS_REFLECT && q.padding_mode <= MI_PS_MINIMUM, "mi_pystripe: padding_mode %d", q.padding_mode);
    // constant padding takes its value from bleach_clip_min also without a frequency: log1p of it (NaN with a frequency: per tile)
    MI_REQUIRE(q.padding_mode != MI_PS_CONSTANT || q.bleach_frequency != 0 || (std::isfinite(q.bleach_clip_min) && q.bleach_clip_min >= 0),
               "mi_pystripe: padding_mode constant pads with log1p(bleach_clip_min); bleach_clip_min %g is not a finite value of 0 or more",
               q.bleach_clip_min);
    MI_REQUIRE(q.down_method >= MI_PS_DOWN_MAX && q.down_method <= MI_PS_DOWN_MEDIAN, "mi_pystripe: down_method %d", q.down_method);
    MI_REQUIRE(q.down_y >= 0 && q.down_x >= 0 && (q.down_y > 0) == (q.down_x > 0), "mi_pystripe: down_sample (%d, %d)", q.down_y, q.down_x);
    MI_REQUIRE(q.rotate == 0 || q.rotate == 90 || q.rotate == 180 || q.rotate == 270, "mi_pystripe: rotate %d (0, 90, 180, 270)", q.rotate);
    MI_REQUIRE(q.level >= 0 && q.level <= MI_PS_MAX_LEVELS, "mi_pystripe: level %d", q.level);
    MI_REQUIRE(!(q.convert_to_16bit && q.convert_to_8bit), "mi_pystripe: convert_to_16bit and convert_to_8bit are both set");
    MI_REQUIRE(!q.convert_to_8bit || (q.bit_shift >= 0 && q.bit_shift <= 8), "right shift should be between 0 and 8 (bit_shift_to_right = %d)",
               q.bit_shift);
    P.in_ny = ny_in; P.in_nx = nx_in; P.in_dtype = in_dtype; P.prm = q;
    mi_pystripe_info& I = P.info;
    std::memset(&I, 0, sizeof I);
    const bool down = q.down_y > 0;
    if (down && q.down_method == MI_PS_DOWN_MEDIAN && (i64)q.down_y * q.down_x > MI_PS_MEDIAN_MAX_BLOCK)
        return fail(MI_ERR_UNSUPPORTED, "mi_pystripe: median down_sample over blocks of %d x %d samples (at most %d samples per block)", q.down_y,
                    q.down_x, MI_PS_MEDIAN_MAX_BLOCK);
    P.pre = down || q.use_flat;
    I.ny = down ? (ny_in + q.down_y - 1) / q.down_y : ny_in;
    I.nx = down ? (nx_in + q.down_x - 1) / q.down_x : nx_in;
    I.integer_kind = in_dtype != MI_PS_F32 && !q.use_flat && !(down && (q.down_method == MI_PS_DOWN_MEAN || q.down_method == MI_PS_DOWN_MEDIAN));
    I.max_batch = q.max_batch > 0 ? q.max_batch : 16;
    // grid limits: rows go to gridDim.y, tiles (twice, in the column synthesis) to gridDim.z
    MI_REQUIRE(I.max_batch <= 16384, "mi_pystripe: max_batch %d (at most 16384 tiles per launch)", I.max_batch);
    P.bleach = q.bleach_frequency != 0;
    // a clip given as NaN is estimated per tile (without a bleach_frequency the three values are not looked at)
    const int au = !P.bleach ? 0 : (std::isnan(q.bleach_clip_min) ? MI_PS_AUTO_MIN : 0) | (std::isnan(q.bleach_clip_med) ? MI_PS_AUTO_MED : 0) |
                                       (std::isnan(q.bleach_clip_max) ? MI_PS_AUTO_MAX : 0);
    P.au = au;
    if (P.bleach) {
        MI_REQUIRE(q.bleach_frequency > 0 && q.bleach_frequency < 1, "mi_pystripe: bleach_frequency %g is not in (0, 1)", q.bleach_frequency);
        // the checks between given clips; an estimated one is checked on the device, tile by tile
        MI_REQUIRE((au & MI_PS_AUTO_MIN) || q.bleach_clip_min >= 0, "mi_pystripe: bleach_clip_min %g is negative", q.bleach_clip_min);
        MI_REQUIRE((au & (MI_PS_AUTO_MIN | MI_PS_AUTO_MED)) || q.bleach_clip_med > q.bleach_clip_min,
                   "mi_pystripe: bleach_clip_med %g is not above bleach_clip_min %g", q.bleach_clip_med, q.bleach_clip_min);
        MI_REQUIRE((au & (MI_PS_AUTO_MED | MI_PS_AUTO_MAX)) || q.bleach_clip_max > q.bleach_clip_med,
                   "mi_pystripe: bleach_clip_max %g is not above bleach_clip_med %g", q.bleach_clip_max, q.bleach_clip_med);
        MI_REQUIRE((au & (MI_PS_AUTO_MIN | MI_PS_AUTO_MAX)) || q.bleach_clip_max > q.bleach_clip_min,
                   "mi_pystripe: bleach_clip_max %g is not above bleach_clip_min %g", q.bleach_clip_max, q.bleach_clip_min);
        // sosfiltfilt's padlen: a filtered line has more than 6 samples
        MI_REQUIRE(I.nx > kBleachExt, "mi_pystripe: bleach correction filters rows of nx = %d samples (after down_sample); at least 7", I.nx);
        MI_REQUIRE(!q.bleach_max_method || I.ny > kBleachExt,
                   "mi_pystripe: bleach_max_method filters the column of ny = %d row maxima (after down_sample); at least 7", I.ny);
        const double k = std::tan(M_PI * q.bleach_frequency / 2.0);
        P.bq.b = k / (1.0 + k);
        P.bq.a = (1.0 - k) / (1.0 + k);
        P.bq.lo = (float)std::max(q.bleach_clip_min, std::log1p(1.0));
        P.bq.med = (float)q.bleach_clip_med;
        P.bq.hi = (float)q.bleach_clip_max;
        P.bq.clips = nullptr;
        P.ncodes = au && I.integer_kind ? (in_dtype == MI_PS_U8 ? 256 : 65536) : 0;
    }
    if (q.log_output) {
        MI_REQUIRE(P.filter || P.bleach, "mi_pystripe: log_output needs a stripe filter (sigma > 0) or the bleach correction");
        I.out_ny = I.ny; I.out_nx = I.nx; I.out_dtype = MI_PS_F32;
    } else {
        const bool swap = q.rotate == 90 || q.rotate == 270;
        I.out_ny = swap ? I.nx : I.ny;
        I.out_nx = swap ? I.ny : I.nx;
        I.out_dtype = q.out_dtype;
    }
    P.passes = !P.filter ? 0 : (q.sigma1 == q.sigma2 ? 1 : 2);
    size_t off = 0;
    auto take = [&off](size_t n) { const size_t o = off; off += (n + 3) / 4 * 4; return o; };
    if (P.pre) { P.sz_stage = (size_t)I.ny * I.nx; P.off_stage = take(P.sz_stage); }
    if (P.filter) {
        I.base_pad = pad_size(I.ny, I.nx, std::max(q.sigma1, q.sigma2));
        I.pad_y = I.ny % 2; I.pad_x = I.nx % 2;
        if (I.ny + 2 * I.base_pad + I.pad_y < kMinLength) I.pad_y = kMinLength - (I.ny + 2 * I.base_pad);
        if (I.nx + 2 * I.base_pad + I.pad_x < kMinLength) I.pad_x = kMinLength - (I.nx + 2 * I.base_pad);
        I.padded_ny = I.ny + 2 * I.base_pad + I.pad_y;
        I.padded_nx = I.nx + 2 * I.base_pad + I.pad_x;
        MI_REQUIRE((i64)I.padded_ny * I.padded_nx < (1ll << 31), "mi_pystripe: padded tile of %d x %d samples", I.padded_ny, I.padded_nx);
        MI_REQUIRE(I.padded_ny <= 65535, "mi_pystripe: padded tile of %d rows (at most 65535)", I.padded_ny);
        // the automatic level is 0 where a padded extent is below L - 1 (never for db9: 34 samples at least): wavedec2 then returns the
        // approximation alone and the filter leaves the log image as it is
        const int L = P.L;
        I.levels = q.level > 0 ? q.level : std::min(max_level(I.padded_ny, L), max_level(I.padded_nx, L));
        P.h[0] = I.padded_ny; P.w[0] = I.padded_nx;
        for (int l = 1; l <= I.levels; ++l) {
            P.h[l] = (P.h[l - 1] + L - 1) / 2;
            P.w[l] = (P.w[l - 1] + L - 1) / 2;
            I.coef_ny[l - 1] = P.h[l]; I.coef_nx[l - 1] = P.w[l];
            // a synthesis pair reads rows p .. p + L / 2 - 1 of a level: s = 2 m - L + 2 outputs need m >= L / 2, true for every
            // m = (n + L - 1) / 2 with n >= 1
            MI_REQUIRE(P.h[l] >= L / 2 && P.w[l] >= L / 2, "mi_pystripe: level %d has %d x %d coefficients", l, P.h[l], P.w[l]);
        }
        // a value padding mode writes the padded image before the first level; an index map never does
        P.valpad = I.levels && q.padding_mode >= MI_PS_CONSTANT;
        if ((P.passes == 2 || P.valpad) && I.levels) { P.sz_P = (size_t)P.h[0] * P.w[0]; P.off_P = take(P.sz_P); }
        if (P.valpad) {
            const int m = q.padding_mode;
            if (m == MI_PS_CONSTANT) P.sz_pvec = (au & MI_PS_AUTO_MIN) ? 1 : 0;
            else if (m != MI_PS_LINEAR_RAMP) P.sz_pvec = (size_t)I.ny + I.nx + 1;
            if (m == MI_PS_MAXIMUM || m == MI_PS_MINIMUM || m == MI_PS_MEAN) P.sz_ppart = 2 * (size_t)I.ny * cdiv(I.nx, 64);
            if (P.sz_pvec) P.off_pvec = take(P.sz_pvec);
            if (P.sz_ppart) P.off_ppart = take(P.sz_ppart);
        }
        // L / H of a level's analysis (h[l - 1] rows of w[l]); lo1 / hi1 of its synthesis (2 h[l] - L + 2 <= h[l - 1] + 1 rows).  The
        // first level is the largest while the extents are L - 1 or more; an explicit level on a shorter extent n GROWS it towards
        // L - 1 ((n + L - 1) / 2 > n), so the largest level is looked for.
        for (int l = 1; l <= I.levels; ++l) P.sz_row = std::max(P.sz_row, (size_t)(P.h[l - 1] + 1) * P.w[l]);
        if (I.levels) {
            P.off_rowL = take(P.sz_row);
            P.off_rowH = take(P.sz_row);
        }
        for (int l = 1; l <= I.levels; ++l) {
            // also holds the reconstruction of level l + 1: with m' = (m + L - 1) / 2, 2 m' - L + 2 <= m + 1 for every L
            P.sz_A[l] = (size_t)(P.h[l] + 1) * (P.w[l] + 1);
            P.sz_d[l] = (size_t)P.h[l] * P.w[l];
            P.off_A[l] = take(P.sz_A[l]);
            P.off_cH[l] = take(P.sz_d[l]);
            P.off_cV[l] = take(P.sz_d[l]);
            P.off_cD[l] = take(P.sz_d[l]);
        }
    }
    if (P.bleach) {
        const size_t npix = (size_t)I.ny * I.nx;
        const int longest = q.bleach_max_method ? std::max(I.ny, I.nx) : I.nx;
        I.bleach_long_rows = longest > MI_PS_BLEACH_LDS_ROW;
        if (P.filter) { P.sz_L = npix; P.off_L = take(P.sz_L); }
        if (q.bleach_max_method) {
            P.sz_vec = (size_t)I.ny + I.nx;
            P.off_key = take(P.sz_vec);
            P.off_vec = take(P.sz_vec);
            if (I.bleach_long_rows) P.sz_fwd = 2 * ((size_t)longest + 2 * kBleachExt);
        } else {
            P.sz_F = npix; P.off_F = take(P.sz_F);
            P.sz_lmax = (size_t)I.ny; P.off_lmax = take(P.sz_lmax);
            if (I.bleach_long_rows) P.sz_fwd = 2 * (size_t)I.ny * ((size_t)I.nx + 2 * kBleachExt);
        }
        P.off_M = take(1);
        if (P.sz_fwd) P.off_fwd = take(P.sz_fwd);
    }
    I.scratch_bytes_per_tile = off * sizeof(float);
    // the output conversion (:1361-1369)
    const int cur = I.integer_kind ? in_dtype : MI_PS_F32;
    if (!q.log_output) {
        if (q.convert_to_16bit && cur != MI_PS_U16)
            MI_REQUIRE(q.out_dtype == MI_PS_U16, "mi_pystripe: convert_to_16bit with out_dtype %d", q.out_dtype);
        else if (q.convert_to_8bit && cur != MI_PS_U8)
            MI_REQUIRE(q.out_dtype == MI_PS_U8, "mi_pystripe: convert_to_8bit with out_dtype %d", q.out_dtype);
    }
    return MI_OK;
}

int check_taps(const char* who, int taps) {
    MI_REQUIRE(taps >= 2 && taps <= MI_PS_MAX_TAPS && taps % 2 == 0, "%s: wavelet of %d taps (an even number, 2 .. %d)", who, taps, MI_PS_MAX_TAPS);
    return MI_OK;
}

// what the plan does to every sample behind the filter
Sink make_sink(const Plan& P, void* out, const int* varies, const int* clip_status) {
    const mi_pystripe_info& I = P.info;
    const mi_pystripe_params& q = P.prm;
    Sink k{};
    k.out = out;
    k.tile_stride = (i64)I.out_ny * I.out_nx;
    k.ny = I.ny; k.nx = I.nx; k.pad = I.base_pad;
    k.filtered = P.filter || P.bleach; k.log_out = q.log_output; k.integer_kind = I.integer_kind;
    k.in_max = P.in_dtype == MI_PS_U8 ? 255.f : 65535.f;
    k.dark = q.dark;
    const int cur = I.integer_kind ? P.in_dtype : MI_PS_F32;
    k.out_dtype = I.out_dtype;
    if (q.convert_to_16bit && cur != MI_PS_U16) { k.mode = OUT_CLIPCAST; k.cast_max = 65535.f; }
    else if (q.convert_to_8bit && cur != MI_PS_U8) { k.mode = OUT_TO8; k.shift = q.bit_shift; }
    else if (I.out_dtype != MI_PS_F32) { k.mode = OUT_CLIPCAST; k.cast_max = I.out_dtype == MI_PS_U8 ? 255.f : 65535.f; }
    else k.mode = OUT_FLOAT;
    k.flip = q.flip_upside_down; k.rot = q.rotate / 90;
    k.varies = varies;
    k.clip_status = clip_status;
    return k;
}

int run_chunk(Plan& P, hipStream_t st, const void* in, const float* flat, void* out, int cnt, i64 t0) {
    const mi_pystripe_info& I = P.info;
    const mi_pystripe_params& q = P.prm;
    int* varies = P.varies.as<int>();
    const i64 npix = (i64)P.in_ny * P.in_nx;
    MI_HIP(hipMemsetAsync(varies, q.keep_uniform ? 1 : 0, sizeof(int) * (size_t)cnt, st));
    if (!q.keep_uniform && !q.log_output) {
        if (P.in_dtype == MI_PS_U16) MI_TRY(launch_uniform<uint16_t>(st, in, npix, cnt, varies));
        else if (P.in_dtype == MI_PS_U8) MI_TRY(launch_uniform<uint8_t>(st, in, npix, cnt, varies));
        else MI_TRY(launch_uniform<float>(st, in, npix, cnt, varies));
    }
    Src src{in, npix, P.in_dtype, P.in_ny, P.in_nx, P.in_nx, 0, MAP_IDENTITY, 0};
    if (P.pre) {
        const int by = q.down_y > 0 ? q.down_y : 1, bx = q.down_x > 0 ? q.down_x : 1;
        const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
        const float* fl = q.use_flat ? flat : nullptr;
        float* stage = P.buf(P.off_stage);
        if (q.down_y > 0 && q.down_method == MI_PS_DOWN_MEDIAN) {
            const int n = by * bx;
            if (n <= 4) MI_TRY(launch_pre_median<4>(st, grid, src, fl, by, bx, stage, I.ny, I.nx));
            else if (n <= 8) MI_TRY(launch_pre_median<8>(st, grid, src, fl, by, bx, stage, I.ny, I.nx));
            else if (n <= 16) MI_TRY(launch_pre_median<16>(st, grid, src, fl, by, bx, stage, I.ny, I.nx));
            else if (n <= 32) MI_TRY(launch_pre_median<32>(st, grid, src, fl, by, bx, stage, I.ny, I.nx));
            else MI_TRY(launch_pre_median<64>(st, grid, src, fl, by, bx, stage, I.ny, I.nx));
        } else {
            hipLaunchKernelGGL(pre_kernel, grid, dim3(256), 0, st, src, fl, by, bx, q.down_method, stage, I.ny, I.nx);
            MI_TRY(launch_check("pre_kernel"));
        }
        src = Src{stage, (i64)P.sz_stage, MI_PS_F32, I.ny, I.nx, I.nx, 0, MAP_IDENTITY, 0};
    }
    const int* clip_status = nullptr;
    if (P.au) {
        float* clips = P.clips_buf.as<float>() + 3 * t0;
        int* status = P.status_buf.as<int>() + t0;
        MI_TRY(run_auto_clips(P, st, src, cnt, varies, clips, status));
        P.bq.clips = clips;
        clip_status = status;
    }
    const Sink k = make_sink(P, out, varies, clip_status);
    if (!P.filter || I.levels == 0) {
        if (P.filter) src.logp = 1;   // no wavelet level: the filter's result is log1p of the tile
        if (P.bleach) {
            src.logp = 1;   // L is log1p on load: no log image is written
            return run_bleach(P, st, src, k, cnt);
        }
        const dim3 grid(cdiv(I.nx, 64), cdiv(I.ny, 4), cnt);
        hipLaunchKernelGGL(point_kernel, grid, dim3(256), 0, st, src, k);
        return launch_check("point_kernel");
    }
    // with the bleach correction behind it, the last synthesis level stores the log image; the correction feeds the real sink
    Sink kL = k;
    if (P.bleach) {
        kL.out = P.buf(P.off_L);
        kL.tile_stride = (i64)P.sz_L;
        kL.log_out = 1;
        kL.clip_status = nullptr;
    }
    const int Lv = I.levels;
    if (P.valpad) MI_TRY(run_value_pad(P, st, src, cnt));
    for (int pass = 0; pass < P.passes; ++pass) {
        // analysis: of the tile through its padding map, of the padded image (a value mode's, or the one the first pass left), or of
        // the level above
        for (int l = 1; l <= Lv; ++l) {
            Src s;
            if (l == 1 && pass == 0 && !P.valpad) {
                s = src;
                s.pad = I.base_pad; s.mode = q.padding_mode; s.logp = 1;
            } else if (l == 1) {
                s = Src{P.buf(P.off_P), (i64)P.sz_P, MI_PS_F32, P.h[0], P.w[0], P.w[0], 0, MAP_IDENTITY, 0};
            } else {
                s = Src{P.buf(P.off_A[l - 1]), (i64)P.sz_A[l - 1], MI_PS_F32, P.h[l - 1], P.w[l - 1], P.w[l - 1], 0, MAP_IDENTITY, 0};
            }
            MI_TRY(launch_analysis(P, st, l, s, cnt));
        }
        // notch
        for (int l = 1; l <= Lv; ++l) {
            const NotchTab* t = &P.tabs[((size_t)pass * Lv + (l - 1)) * 2];
            MI_TRY(run_notch(P, st, t[0], P.buf(P.off_cH[l]), (i64)P.sz_d[l], P.h[l], 1, P.w[l], cnt));
            if (q.bidirectional) MI_TRY(run_notch(P, st, t[1], P.buf(P.off_cV[l]), (i64)P.sz_d[l], P.w[l], P.w[l], 1, cnt));
        }
        // synthesis, deepest level first; the last level of the last pass goes through the sink
        for (int l = Lv; l >= 1; --l) MI_TRY(launch_synthesis(P, st, l, l == 1 && pass == P.passes - 1, kL, cnt));
    }
    if (P.bleach)
        return run_bleach(P, st, Src{P.buf(P.off_L), (i64)P.sz_L, MI_PS_F32, I.ny, I.nx, I.nx, 0, MAP_IDENTITY, 0}, k, cnt);
    return MI_OK;
}

// rec_lo == null: db9 through its own kernels (taps is 0); else the wavelet of that low-pass through the generic ones
int create_plan(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params& q, const double* rec_lo, int taps, void** plan) {
    MI_TRY(use_device(dev));
    Plan* P = new Plan;
    P->dev = dev;
    if (!rec_lo) P->f = make_filters();
    int rc = derive(ny, nx, in_dtype, q, taps, *P);
    if (rc == MI_OK) rc = build_tables(*P);
    if (rc == MI_OK && rec_lo) rc = upload_filter_table(*P, rec_lo);
    if (rc == MI_OK) rc = upload_log_table(*P, nullptr);
    if (rc != MI_OK) {
        delete P;
        return rc;
    }
    *plan = P;
    return MI_OK;
}

int derive_info(int ny, int nx, int in_dtype, const mi_pystripe_params& q, int taps, mi_pystripe_info* info) {
    Plan P;
    MI_TRY(derive(ny, nx, in_dtype, q, taps, P));
    *info = P.info;
    return MI_OK;
}

}  // namespace
}  // namespace ps
}  // namespace mi

using namespace mi::ps;

extern "C" int mi_pystripe_pad_size(int ny, int nx, double sigma) {
    if (ny <= 0 || nx <= 0 || sigma < 0) return mi::fail(MI_ERR_INVALID, "mi_pystripe_pad_size: shape (%d, %d), sigma %g", ny, nx, sigma);
    return pad_size(ny, nx, sigma);
}

extern "C" int mi_pystripe_derive(int ny, int nx, int in_dtype, const mi_pystripe_params* params, mi_pystripe_info* info) {
    MI_REQUIRE(params && info, "mi_pystripe_derive: null pointer");
    return derive_info(ny, nx, in_dtype, *params, 0, info);
}

extern "C" int mi_pystripe_plan_create(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, void** plan) {
    MI_REQUIRE(params && plan, "mi_pystripe_plan_create: null pointer");
    *plan = nullptr;
    return create_plan(dev, ny, nx, in_dtype, *params, nullptr, 0, plan);
}

extern "C" int mi_pystripe_derive_wavelet(int ny, int nx, int in_dtype, const mi_pystripe_params* params, int taps, mi_pystripe_info* info) {
    MI_REQUIRE(params && info, "mi_pystripe_derive_wavelet: null pointer");
    MI_TRY(check_taps("mi_pystripe_derive_wavelet", taps));
    return derive_info(ny, nx, in_dtype, *params, taps, info);
}

extern "C" int mi_pystripe_plan_create_wavelet(int dev, int ny, int nx, int in_dtype, const mi_pystripe_params* params, const double* rec_lo,
                                               int taps, void** plan) {
    MI_REQUIRE(params && plan && rec_lo, "mi_pystripe_plan_create_wavelet: null pointer");
    *plan = nullptr;
    MI_TRY(check_taps("mi_pystripe_plan_create_wavelet", taps));
    // orthonormal under double shifts: what the quadrature-mirror construction of the other three filters needs
    for (int i = 0; i < taps; ++i) MI_REQUIRE(std::isfinite(rec_lo[i]), "mi_pystripe_plan_create_wavelet: rec_lo[%d] is not finite", i);
    double worst = 0.0;
    for (int k = 0; 2 * k < taps; ++k) {
        double sum = 0.0;
        for (int i = 0; i + 2 * k < taps; ++i) sum += rec_lo[i] * rec_lo[i + 2 * k];
        worst = std::max(worst, std::fabs(sum - (k == 0 ? 1.0 : 0.0)));
    }
    MI_REQUIRE(worst <= 1e-6, "mi_pystripe_plan_create_wavelet: rec_lo is not the low-pass of an orthogonal wavelet (residual %g, allowed 1e-6)",
               worst);
    return create_plan(dev, ny, nx, in_dtype, *params, rec_lo, taps, plan);
}

extern "C" int mi_pystripe_plan_destroy(void* plan) {
    if (!plan) return MI_OK;
    Plan* P = static_cast<Plan*>(plan);
    const int rc = mi::use_device(P->dev);
    delete P;
    return rc;
}

extern "C" int mi_pystripe_plan_info(void* plan, mi_pystripe_info* info) {
    MI_REQUIRE(plan && info, "mi_pystripe_plan_info: null pointer");
    *info = static_cast<Plan*>(plan)->info;
    return MI_OK;
}

extern "C" int mi_pystripe_plan_notch_routes(void* plan, int* out, int cap) {
    MI_REQUIRE(plan, "mi_pystripe_plan_notch_routes: null pointer");
    const Plan& P = *static_cast<Plan*>(plan);
    const int count = (int)P.tabs.size();
    MI_REQUIRE(cap >= 0 && (i64)count * MI_PS_NOTCH_ROUTE_INTS <= (i64)cap && (out || count == 0),
               "mi_pystripe_plan_notch_routes: cap = %d ints, the plan's %d records need %d", cap, count, count * MI_PS_NOTCH_ROUTE_INTS);
    const int Lv = P.info.levels;
    for (int i = 0; i < count; ++i) {
        const NotchTab& t = P.tabs[i];   // build_tables: [pass][level 1..L][axis]
        const int rec[MI_PS_NOTCH_ROUTE_INTS] = {i / (2 * Lv), (i / 2) % Lv + 1, i % 2, t.n, t.kp, t.kb, t.R, t.threads, (int)t.lds};
        std::copy(rec, rec + MI_PS_NOTCH_ROUTE_INTS, out + (size_t)i * MI_PS_NOTCH_ROUTE_INTS);
    }
    return count;
}

extern "C" int mi_pystripe_plan_set_log_table(void* plan, const float* table, int ncodes) {
    MI_REQUIRE(plan && table, "mi_pystripe_plan_set_log_table: null pointer");
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(P.ncodes > 0, "mi_pystripe_plan_set_log_table: the plan estimates no clips of an integer tile");
    MI_REQUIRE(ncodes == P.ncodes, "mi_pystripe_plan_set_log_table: %d codes, the plan's tiles have %d", ncodes, P.ncodes);
    MI_TRY(mi::use_device(P.dev));
    MI_HIP(hipDeviceSynchronize());   // a run that reads the table may still be under way
    return upload_log_table(P, table);
}

extern "C" int mi_pystripe_plan_clips(void* plan, float* clips_host, int* status_host, int n) {
    MI_REQUIRE(plan, "mi_pystripe_plan_clips: null pointer");
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(P.bleach, "mi_pystripe_plan_clips: the plan has no bleach correction");
    MI_REQUIRE(n >= 0 && n <= P.last_count, "mi_pystripe_plan_clips: %d tiles, the last run had %lld", n, (long long)P.last_count);
    if (n == 0) return MI_OK;
    if (!P.au) {
        for (int t = 0; t < n; ++t) {
            if (clips_host) { clips_host[3 * t] = P.bq.lo; clips_host[3 * t + 1] = P.bq.med; clips_host[3 * t + 2] = P.bq.hi; }
            if (status_host) status_host[t] = MI_PS_CLIPS_OK;
        }
        return MI_OK;
    }
    MI_TRY(mi::use_device(P.dev));
    if (clips_host) MI_HIP(hipMemcpy(clips_host, P.clips_buf.p, 3 * sizeof(float) * (size_t)n, hipMemcpyDeviceToHost));
    if (status_host) MI_HIP(hipMemcpy(status_host, P.status_buf.p, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost));
    return MI_OK;
}

extern "C" int mi_pystripe_run(void* plan, void* stream, const void* in, const void* flat, void* out, int64_t count) {
    MI_REQUIRE(plan && in && out, "mi_pystripe_run: null pointer");
    MI_REQUIRE(count >= 0, "mi_pystripe_run: count %lld", (long long)count);
    Plan& P = *static_cast<Plan*>(plan);
    MI_REQUIRE(!P.prm.use_flat || flat, "mi_pystripe_run: the plan divides by a flat field and none is given");
    if (count == 0) return MI_OK;
    MI_TRY(mi::use_device(P.dev));
    hipStream_t st = mi::as_stream(stream);
    const int64_t want = std::min<int64_t>(count, P.info.max_batch);
    if (want > P.cap) {
        // work of an earlier call may still use the smaller scratch
        MI_HIP(hipStreamSynchronize(st));
        P.cap = 0;
        MI_TRY(P.scratch.alloc(std::max<size_t>(P.info.scratch_bytes_per_tile * (size_t)want, 16)));
        MI_TRY(P.varies.alloc(sizeof(int) * (size_t)want));
        if (P.au) MI_TRY(P.auto_buf.alloc(kAutoBytesPerTile * (size_t)want));
        P.cap = want;
    }
    if (P.au && count > P.clips_cap) {
        MI_HIP(hipStreamSynchronize(st));
        P.clips_cap = 0;
        MI_TRY(P.clips_buf.alloc(3 * sizeof(float) * (size_t)count));
        MI_TRY(P.status_buf.alloc(sizeof(int) * (size_t)count));
        P.clips_cap = count;
    }
    P.last_count = count;
    const size_t in_bytes = (size_t)P.in_ny * P.in_nx * (P.in_dtype == MI_PS_U8 ? 1 : P.in_dtype == MI_PS_U16 ? 2 : 4);
    const size_t out_bytes = (size_t)P.info.out_ny * P.info.out_nx * (P.info.out_dtype == MI_PS_U8 ? 1 : P.info.out_dtype == MI_PS_U16 ? 2 : 4);
    for (int64_t t0 = 0; t0 < count; t0 += P.cap) {
        const int cnt = (int)std::min<int64_t>(P.cap, count - t0);
        MI_TRY(run_chunk(P, st, static_cast<const char*>(in) + (size_t)t0 * in_bytes, static_cast<const float*>(flat),
                         static_cast<char*>(out) + (size_t)t0 * out_bytes, cnt, t0));
    }
    return MI_OK;
}
