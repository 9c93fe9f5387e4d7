// Device-side text the pystripe units share: where a sample comes from (Src), the padding map it is read through, and what
// happens to it behind the filter (Sink).  Host side and the map of the units: pystripe_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mi_pystripe.h"
#include "thresholds_dev.h"
#include "wavelet_db9.h"

namespace mi {
namespace ps {

using namespace db9;
using histdev::float_key;   // order-preserving keys of floats
using histdev::key_float;
using i64 = long long;

enum { MAP_IDENTITY = -1 };   // Src::mode beside the index maps of mi_pystripe_padding: the image is read as it lies
enum { SRC_KEY = 3 };   // Src::dtype beside mi_pystripe_dtype: order-preserving keys of floats (float_key)
enum { OUT_FLOAT = 0, OUT_TO8 = 1, OUT_CLIPCAST = 2 };

// numpy.pad's index map: padded coordinate i (pad samples in front) -> source index in [0, n)
__device__ __forceinline__ int pad_index(int i, int pad, int n, int mode) {
    int q = i - pad;
    if (mode == MAP_IDENTITY || (q >= 0 && q < n)) return q;
    if (mode == MI_PS_EDGE) return q < 0 ? 0 : n - 1;
    if (mode == MI_PS_WRAP) {
        q %= n;
        return q < 0 ? q + n : q;
    }
    if (mode == MI_PS_SYMMETRIC) return sym_index(q, n);
    if (n == 1) return 0;   // reflect
    const int p = 2 * n - 2;
    q %= p;
    if (q < 0) q += p;
    return q < n ? q : p - q;
}

// where a level's input comes from: the tile itself (any dtype, through the padding map, log1p) or a float image of the pyramid
struct Src {
    const void* p;
    i64 tile_stride;   // samples
    int dtype, ny, nx, row_stride;
    int pad, mode, logp;
};

__device__ __forceinline__ float src_load(const Src& s, i64 tile, int y, int x) {
    const i64 o = tile * s.tile_stride + (i64)y * s.row_stride + x;
    float v;
    if (s.dtype == MI_PS_U16) v = (float)static_cast<const uint16_t*>(s.p)[o];
    else if (s.dtype == MI_PS_U8) v = (float)static_cast<const uint8_t*>(s.p)[o];
    else if (s.dtype == SRC_KEY) v = key_float(static_cast<const unsigned*>(s.p)[o]);
    else v = static_cast<const float*>(s.p)[o];
    return s.logp ? log1pf(v) : v;
}

// what happens to a sample after the filter (process_img :1322-1379 and the tail of filter_streaks :1150-1158)
struct Sink {
    void* out;
    i64 tile_stride;        // samples
    int ny, nx;             // the un-padded tile
    int pad;                // rows / columns in front of it in the padded image
    int filtered;           // the value is in the log domain: expm1 (and rint + clip for integer tiles)
    int log_out;
    int integer_kind;
    float in_max;
    float dark;
    int mode, shift, out_dtype;
    float cast_max;
    int flip, rot;
    const int* varies;      // per tile: 0 = uniform tile -> zeros
    const int* clip_status; // automatic clips: per tile, > 0 = no usable clips -> zeros, also in the log output; else null
};

__device__ __forceinline__ void sink_store(const Sink& k, i64 tile, int y, int x, float v) {
    if (k.log_out) {
        if (k.clip_status && k.clip_status[tile] > 0) v = 0.f;
        static_cast<float*>(k.out)[tile * k.tile_stride + (i64)y * k.nx + x] = v;
        return;
    }
    if (k.filtered) {
        v = expm1f(v);
        if (k.integer_kind) v = fminf(fmaxf(rintf(v), 0.f), k.in_max);
    }
    if (k.dark > 0.f) {
        v = v > k.dark ? v - k.dark : 0.f;
        if (k.integer_kind) v = truncf(v);
    }
    if (!k.varies[tile]) v = 0.f;
    if (k.flip) y = k.ny - 1 - y;
    int oy = y, ox = x, onx = k.nx;
    if (k.rot == 1) { oy = k.nx - 1 - x; ox = y; onx = k.ny; }
    else if (k.rot == 2) { oy = k.ny - 1 - y; ox = k.nx - 1 - x; }
    else if (k.rot == 3) { oy = x; ox = k.ny - 1 - y; onx = k.ny; }
    const i64 o = tile * k.tile_stride + (i64)oy * onx + ox;
    if (k.mode == OUT_FLOAT) {
        static_cast<float*>(k.out)[o] = v;
        return;
    }
    int u;
    if (k.mode == OUT_TO8) {
        u = (int)fminf(fmaxf(v, 0.f), 65535.f);
        u = (u > 0 && u < (1 << k.shift)) ? 1 : (u >> k.shift);
        u = min(u, 255);
    } else {
        u = (int)fminf(fmaxf(v, 0.f), k.cast_max);
    }
    if (k.out_dtype == MI_PS_U16) static_cast<uint16_t*>(k.out)[o] = (uint16_t)u;
    else static_cast<uint8_t*>(k.out)[o] = (uint8_t)u;
}

}  // namespace ps
}  // namespace mi
