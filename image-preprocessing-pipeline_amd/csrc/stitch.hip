// Stitching step 6 (include/mi_stitch.h): the merge of a grid of placed stacks into the stitched volume.
//
// The host restates the reference's bookkeeping once per call and hands the kernel small tables; the kernel makes one pass
// over the output box, each lane eight consecutive columns of one row:
//   ST   per stripe (row of stacks) and stripe column: which stack writes it, whether it lies in the H overlap with the stack
//        on its left and at which step of the blend (StackStitcher::getStripe2, StackStitcher.cpp:1854-2140)
//   CT   per pair of adjacent stripes and output column: the rows copied from the upper stripe, blended, copied from the lower
//        one (the corner walk of UnstitchedVolume::internal_loadSubvolume_to_real32, UnstitchedVolume.cpp:596-899, including
//        the stale h of the last corners and the rule of the last region)
//   YR   per output row: the stripes whose zones contain it (normally one), and the stripe it is a plain row of (no V overlap)
//   W    blend weights per overlap length: (cos(angle)+1)*0.5 with the angle accumulated in double, 0..PI in PI/(n-1) steps
// Plain copies outside overlaps are exact (v / 65535.0F * 65535.0F == v for every 16-bit and 8-bit sample); overlap voxels
// are blended in double in the reference's expression order, with contraction off.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <map>
#include <vector>

#include "mi_internal.h"
#include "mi_stitch.h"

namespace {

constexpr double kPI = 3.14159265;   // IM_config.h:149 (the constant of the blend angle step)
constexpr double kSPI = 3.14159265;  // S_config.h:48 (no_blending's threshold)
constexpr int kVec = 8;              // output columns per lane
constexpr int kNone = 0xFF;
constexpr int kCT = 8;               // ints per CT entry: ua ub oa ob da db wbase pad

struct Params {
    const double* W;
    const unsigned long long* stk;   // device pointers of the stacks, row-major
    const int* rc;                   // per stack: vtop (ABS_V - stripe top), hleft (ABS_H - stripe left), H-blend weight base
    const int* row;                  // per stripe: dtop, dleft, Hr, Wr, brh (absolute right edge), na, nb, st offset
    const int* ST;
    const int* CT;
    const int4* YR;
    int R, C, Hs, Ws, Wv;            // grid, stack size, volume width
    int bytes, blending;
    int D0, V0, H0, Vb, Hb;          // output box origin and size (rows, columns)
    float scale;
};

__device__ __forceinline__ float sample(const Params& p, int s, int zrel, int i, int j) {
    const size_t off = ((size_t)zrel * p.Hs + i) * p.Ws + j;
    const unsigned v = p.bytes == 2 ? reinterpret_cast<const uint16_t*>(p.stk[s])[off] : reinterpret_cast<const uint8_t*>(p.stk[s])[off];
    return (float)v / p.scale;
}

__device__ __forceinline__ float blend(const Params& p, double w, float p1, float p2) {
#pragma clang fp contract(off)
    if (p.blending == MI_NOBLEND) return w != 0.0 ? p1 : p2;
    if (p1 == 0.0f || p2 == 0.0f) return p1 < p2 ? p2 : p1;   // black pixels are ignored (std::max)
    const double a = w * (double)p1;
    const double b = (1.0 - w) * (double)p2;
    return (float)(a + b);
}

// value of stripe r at (i, j): a pointer walk past the end of a stripe row continues on the next row (as the reference's)
__device__ float stripe_val(const Params& p, int r, int zrel, int i, int j) {
    const int* rw = p.row + 8 * r;
    const int Hr = rw[2], Wr = rw[3];
    if (i < 0 || i >= Hr || j < 0 || j >= Wr) {
        const long long f = (long long)i * Wr + j;
        if (f < 0 || f >= (long long)Hr * Wr) return 0.0f;
        i = (int)(f / Wr);
        j = (int)(f % Wr);
    }
    const int e = p.ST[rw[7] + j];
    const int cr = e & 0xFF;
    if (cr == kNone) return 0.0f;
    const int cl = (e >> 8) & 0xFF;
    const int sr = r * p.C + cr;
    const int ri = i - p.rc[3 * sr];
    const bool rv = ri >= 0 && ri < p.Hs;
    const float pr = rv ? sample(p, sr, zrel, ri, j - p.rc[3 * sr + 1]) : 0.0f;
    if (cl == kNone) return pr;
    const int sl = r * p.C + cl;
    const int li = i - p.rc[3 * sl];
    const bool lv = li >= 0 && li < p.Hs;
    if (!lv) return pr;
    const float pl = sample(p, sl, zrel, li, j - p.rc[3 * sl + 1]);
    if (!rv) return pl;
    return blend(p, p.W[p.rc[3 * sr + 2] + (e >> 16)], pl, pr);
}

__device__ float merged_val(const Params& p, int zrel, int Y, int X) {
    const int4 yr = p.YR[Y];
    float v = 0.0f;
    for (int r = yr.x; r <= yr.y; ++r) {
        const int* rw = p.row + 8 * r;
        if (r >= 1) {
            const int* ct = p.CT + ((size_t)(r - 1) * p.Wv + X) * kCT;
            const int* uw = rw - 8;
            if (Y >= ct[0] && Y < ct[1]) v = stripe_val(p, r - 1, zrel, Y - uw[0], X - uw[1]);
            if (Y >= ct[2] && Y < ct[3])
                v = blend(p, p.W[ct[6] + (Y - ct[2])], stripe_val(p, r - 1, zrel, Y - uw[0], X - uw[1]),
                          stripe_val(p, r, zrel, Y - rw[0], X - rw[1]));
            if (Y >= ct[4] && Y < ct[5]) v = stripe_val(p, r, zrel, Y - rw[0], X - rw[1]);
        }
        if (Y >= rw[5] && Y < rw[6]) {
            const int jj = X - rw[1];
            if (jj >= 0 && jj < rw[4]) v = stripe_val(p, r, zrel, Y - rw[0], jj);
        }
    }
    return v;
}

__device__ __forceinline__ unsigned to_sample(float v, float scale) {
    const float f = v * scale;
    return f == f ? (unsigned)(int)f : 0u;       // NaN: what x86's cvttss2si leaves in the low bits
}

// The common case: a plain row whose n columns all lie in the copy zone of one stack of the stripe -- the samples themselves
// (v / scale * scale == v for every sample), no tables beyond two stripe entries, no float.  False: take the general path.
__device__ __forceinline__ bool copy_run(const Params& p, int zrel, int Y, int X, int n, unsigned* q) {
    const int r = p.YR[Y].z;
    if (r < 0) return false;
    const int* rw = p.row + 8 * r;
    const int j0 = X - rw[1], i = Y - rw[0];
    if (j0 < 0 || j0 + n > rw[3] || j0 + n > rw[4] || i < 0 || i >= rw[2]) return false;
    const int e0 = p.ST[rw[7] + j0], e1 = p.ST[rw[7] + j0 + n - 1];
    if (e0 != ((e0 & 0xFF) | (kNone << 8)) || (e1 & 0xFFFF) != (e0 & 0xFFFF) || (e0 & 0xFF) == kNone) return false;
    const int s = r * p.C + (e0 & 0xFF);
    const int ri = i - p.rc[3 * s];
    if (ri < 0 || ri >= p.Hs) {
        for (int k = 0; k < kVec; ++k) q[k] = 0u;
        return true;
    }
    const size_t off = ((size_t)zrel * p.Hs + ri) * p.Ws + (j0 - p.rc[3 * s + 1]);
    if (p.bytes == 2) {
        const uint16_t* src = reinterpret_cast<const uint16_t*>(p.stk[s]) + off;
#pragma unroll
        for (int k = 0; k < kVec; ++k) q[k] = k < n ? src[k] : 0u;
    } else {
        const uint8_t* src = reinterpret_cast<const uint8_t*>(p.stk[s]) + off;
#pragma unroll
        for (int k = 0; k < kVec; ++k) q[k] = k < n ? src[k] : 0u;
    }
    return true;
}

__global__ void __launch_bounds__(256) merge_kernel(Params p, void* out) {
    const int x0 = (blockIdx.x * blockDim.x + threadIdx.x) * kVec;
    const int y = blockIdx.y;
    const int zrel = blockIdx.z;
    if (x0 >= p.Hb) return;
    const int Y = p.V0 + y;
    const size_t base = ((size_t)zrel * p.Vb + y) * p.Hb + x0;
    const int n = min(kVec, p.Hb - x0);
    unsigned q[kVec];
    if (!copy_run(p, zrel, Y, p.H0 + x0, n, q)) {
#pragma unroll
        for (int k = 0; k < kVec; ++k) q[k] = k < n ? to_sample(merged_val(p, zrel, Y, p.H0 + x0 + k), p.scale) : 0u;
    }
    if (p.bytes == 2) {
        uint16_t* o = reinterpret_cast<uint16_t*>(out) + base;
        if (n == kVec && (reinterpret_cast<uintptr_t>(o) & 15) == 0) {
            uint4 w;
            w.x = q[0] | (q[1] << 16);
            w.y = q[2] | (q[3] << 16);
            w.z = q[4] | (q[5] << 16);
            w.w = q[6] | (q[7] << 16);
            *reinterpret_cast<uint4*>(o) = w;
        } else {
            for (int k = 0; k < n; ++k) o[k] = (uint16_t)q[k];
        }
    } else {
        uint8_t* o = reinterpret_cast<uint8_t*>(out) + base;
        if (n == kVec && (reinterpret_cast<uintptr_t>(o) & 7) == 0) {
            uint2 w;
            w.x = (q[0] & 0xFF) | ((q[1] & 0xFF) << 8) | ((q[2] & 0xFF) << 16) | (q[3] << 24);
            w.y = (q[4] & 0xFF) | ((q[5] & 0xFF) << 8) | ((q[6] & 0xFF) << 16) | (q[7] << 24);
            *reinterpret_cast<uint2*>(o) = w;
        } else {
            for (int k = 0; k < n; ++k) o[k] = (uint8_t)q[k];
        }
    }
}

struct Dims { int V0, V1, H0, H1, D0, D1; };

Dims volume_dims(int R, int C, const int* av, const int* ah, const int* ad, int Hs, int Ws, int N) {
    Dims d{std::numeric_limits<int>::max(), std::numeric_limits<int>::min(), std::numeric_limits<int>::max(),
           std::numeric_limits<int>::min(), std::numeric_limits<int>::min(), std::numeric_limits<int>::max()};
    for (int j = 0; j < C; ++j) {
        d.V0 = std::min(d.V0, av[j]);
        d.V1 = std::max(d.V1, av[(R - 1) * C + j]);
    }
    for (int i = 0; i < R; ++i) {
        d.H0 = std::min(d.H0, ah[i * C]);
        d.H1 = std::max(d.H1, ah[i * C + C - 1]);
    }
    for (int s = 0; s < R * C; ++s) {
        d.D0 = std::max(d.D0, ad[s]);
        d.D1 = std::min(d.D1, ad[s]);
    }
    d.V1 += Hs;
    d.H1 += Ws;
    d.D1 += N;
    return d;
}

// the weight table of one overlap length n: the angle starts at 0 and adds PI/(n-1) per step, in double (the division by
// zero of n == 1 gives inf as in C; only the first step is ever used then)
struct Weights {
    std::vector<double> w;
    std::map<int, int> base;
    int blending;
    int get(int n) {
        auto it = base.find(n);
        if (it != base.end()) return it->second;
        const int b = (int)w.size();
        const int cnt = std::max(n, 1);
        const double delta = kPI / (double)(n - 1);
        double angle = 0;
        for (int t = 0; t < cnt; ++t) {
            if (blending == MI_NOBLEND)
                w.push_back(angle <= kSPI / 2 ? 1.0 : 0.0);
            else
                w.push_back(std::isfinite(angle) ? (std::cos(angle) + 1.0F) * 0.5F : std::numeric_limits<double>::quiet_NaN());
            angle = angle + delta;
        }
        base[n] = b;
        return b;
    }
};

struct Corner { int H, h; bool up; };

}  // namespace

extern "C" int mi_merge_volume_dims(int n_rows, int n_cols, const int* abs_v, const int* abs_h, const int* abs_d, int height, int width,
                                    int n_slices, int* dims) {
    MI_REQUIRE(n_rows > 0 && n_cols > 0 && abs_v && abs_h && abs_d && dims && height > 0 && width > 0 && n_slices > 0,
               "mi_merge_volume_dims: bad arguments");
    const Dims d = volume_dims(n_rows, n_cols, abs_v, abs_h, abs_d, height, width, n_slices);
    const int v[6] = {d.V0, d.V1, d.H0, d.H1, d.D0, d.D1};
    std::memcpy(dims, v, sizeof v);
    return MI_OK;
}

extern "C" int mi_merge_slab(int dev, void* stream, int R, int C, const int* av, const int* ah, const int* ad, int Hs, int Ws, int N,
                             const void* const* stacks, int bytes, int blending, int D0, int D1, int V0, int V1, int H0, int H1,
                             void* out) {
    MI_REQUIRE(R > 0 && C > 0 && R < kNone && C < kNone, "mi_merge_slab: grid %d x %d out of range [1,254]", R, C);
    MI_REQUIRE(av && ah && ad && stacks && out, "mi_merge_slab: null pointer");
    MI_REQUIRE(Hs > 0 && Ws > 0 && N > 0, "mi_merge_slab: stacks of %d x %d x %d", Hs, Ws, N);
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_merge_slab: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(blending == MI_SINBLEND || blending == MI_NOBLEND, "mi_merge_slab: blending %d (SINBLEND 0, NOBLEND 1)", blending);
    for (int i = 0; i < R; ++i)
        for (int j = 0; j + 1 < C; ++j)
            MI_REQUIRE(ah[i * C + j] < ah[i * C + j + 1], "mi_merge_slab: ABS_H of row %d does not increase at column %d", i, j);
    const Dims d = volume_dims(R, C, av, ah, ad, Hs, Ws, N);
    const int Hv = d.V1 - d.V0, Wv = d.H1 - d.H0, Dv = d.D1 - d.D0;
    MI_REQUIRE(Hv > 0 && Wv > 0 && Dv > 0, "mi_merge_slab: empty volume (%d x %d x %d): the stacks share no slice", Hv, Wv, Dv);
    MI_REQUIRE(0 <= D0 && D0 < D1 && D1 <= Dv && 0 <= V0 && V0 < V1 && V1 <= Hv && 0 <= H0 && H0 < H1 && H1 <= Wv,
               "mi_merge_slab: box [%d,%d) x [%d,%d) x [%d,%d) outside the volume %d x %d x %d", D0, D1, V0, V1, H0, H1, Dv, Hv, Wv);
    MI_REQUIRE(D1 - D0 <= 65535 && V1 - V0 <= 65535, "mi_merge_slab: box of %d slices x %d rows (at most 65535 each)", D1 - D0, V1 - V0);
    for (int s = 0; s < R * C; ++s) MI_REQUIRE(stacks[s], "mi_merge_slab: stack %d has no samples", s);

    Weights W;
    W.blending = blending;
    // per stripe (getStripe2 of the whole row)
    std::vector<int> row(8 * R), rc(3 * R * C), ST;
    std::vector<int> ulv(R), brv(R), ulh(R), brh(R);
    for (int r = 0; r < R; ++r) {
        int top = av[r * C], bot = av[r * C];
        for (int c = 1; c < C; ++c) {
            top = std::min(top, av[r * C + c]);
            bot = std::max(bot, av[r * C + c]);
        }
        ulv[r] = top;
        brv[r] = bot + Hs;
        ulh[r] = ah[r * C];
        brh[r] = ah[r * C + C - 1] + Ws;
    }
    for (int r = 0; r < R; ++r) {
        const int Hr = brv[r] - ulv[r], Wr = brh[r] - ulh[r];
        MI_REQUIRE(Wr < (1 << 30), "mi_merge_slab: stripe %d too wide", r);
        const int st = (int)ST.size();
        ST.resize(st + Wr, kNone | (kNone << 8));
        for (int c = 0; c < C; ++c) {
            const int s = r * C + c;
            rc[3 * s] = av[s] - ulv[r];
            rc[3 * s + 1] = ah[s] - ulh[r];
            const int r_left = ah[s] - ulh[r];
            const bool l = c > 0, rr = c < C - 1;
            const int l_right = l ? ah[s - 1] - ulh[r] + Ws : 0;
            if (l) {
                const int n = ah[s - 1] + Ws - ah[s];
                MI_REQUIRE(n < 65536, "mi_merge_slab: H overlap of %d columns", n);
                rc[3 * s + 2] = W.get(n);
            }
            const int j_end = rr ? std::min(ah[s + 1] - ulh[r], r_left + Ws) : Wr;
            for (int j = l ? r_left : 0; j < j_end; ++j) {
                if (j < 0 || j >= Wr) continue;
                if (l && j < l_right)
                    ST[st + j] = c | ((c - 1) << 8) | ((j - r_left) << 16);
                else
                    ST[st + j] = c | (kNone << 8);
            }
        }
        int* rw = &row[8 * r];
        rw[0] = ulv[r] - d.V0;
        rw[1] = ulh[r] - d.H0;
        rw[2] = Hr;
        rw[3] = Wr;
        rw[4] = brh[r];                              // the absolute edge the non-overlapping copy compares with (:879)
        rw[5] = r == 0 ? 0 : brv[r - 1] - d.V0;
        rw[6] = r == R - 1 ? Hv : ulv[r + 1] - d.V0;
        rw[7] = st;
    }
    // corners (UnstitchedVolume.cpp:596-672) and the column table of every pair of stripes
    std::vector<int> CT((size_t)std::max(R - 1, 0) * Wv * kCT, 0);
    std::vector<int> span_lo(R, std::numeric_limits<int>::max()), span_hi(R, std::numeric_limits<int>::min());
    {
        std::vector<std::vector<Corner>> ups(R), bots(R);
        for (int r = 0; r < R; ++r) {
            Corner t;
            t.H = ah[r * C];
            t.h = av[r * C] - ulv[r];
            t.up = true;
            ups[r].push_back(t);
            t.h = brv[r] - av[r * C] - Hs;
            t.up = false;
            bots[r].push_back(t);
            for (int c = 0; c + 1 < C; ++c) {
                const int s = r * C + c;
                if (av[s] < av[s + 1]) {
                    t.H = ah[s] + Ws; t.h = av[s + 1] - ulv[r]; t.up = true; ups[r].push_back(t);
                    t.H = ah[s + 1]; t.h = brv[r] - av[s + 1] - Hs; t.up = false; bots[r].push_back(t);
                } else {
                    t.H = ah[s + 1]; t.h = av[s + 1] - ulv[r]; t.up = true; ups[r].push_back(t);
                    t.H = ah[s] + Ws; t.h = brv[r] - av[s + 1] - Hs; t.up = false; bots[r].push_back(t);
                }
            }
            t.H = ah[r * C + C - 1] + Ws;
            t.up = true;
            ups[r].push_back(t);
            t.up = false;
            bots[r].push_back(t);
        }
        for (int r = 1; r < R; ++r) {
            std::vector<Corner> m;   // std::list::merge: stable, the bottoms of the upper stripe first on equal H
            size_t i = 0, k = 0;
            const auto& a = bots[r - 1];
            const auto& b = ups[r];
            while (i < a.size() || k < b.size()) {
                if (k >= b.size() || (i < a.size() && !(b[k].H < a[i].H))) m.push_back(a[i++]);
                else m.push_back(b[k++]);
            }
            const long long d_top = ulv[r] - d.V0, u_bottom = brv[r - 1] - d.V0;
            const long long ov = u_bottom - d_top;
            long long h_up = ov, h_down = ov;
            for (size_t q = 0; q + 1 < m.size(); ++q) {
                const Corner& cl = m[q];
                const Corner& cr = m[q + 1];
                if (q + 2 == m.size()) {
                    h_up = cl.up ? ov : 0;
                    h_down = cl.up ? 0 : ov;
                } else if (cl.up) {
                    h_up = cl.h;
                } else {
                    h_down = cl.h;
                }
                const long long h_ov = ov - h_up - h_down;
                int e[kCT];
                e[0] = (int)d_top;
                e[1] = (int)std::min(d_top + h_up + (h_ov >= 0 ? 0 : h_ov), (long long)Hv);
                e[2] = (int)(d_top + h_up);
                e[3] = (int)std::min(d_top + h_up + h_ov, (long long)Hv);
                e[4] = (int)(d_top + h_up + (h_ov >= 0 ? h_ov : 0));
                e[5] = (int)std::min(d_top + h_up + h_ov + h_down, (long long)Hv);
                e[6] = e[3] > e[2] ? W.get((int)h_ov) : 0;
                e[7] = 0;
                for (int z = 0; z < 3; ++z)
                    if (e[2 * z + 1] > e[2 * z]) {
                        span_lo[r] = std::min(span_lo[r], e[2 * z]);
                        span_hi[r] = std::max(span_hi[r], e[2 * z + 1]);
                    }
                for (int j = std::max(cl.H - d.H0, 0); j < std::min(cr.H - d.H0, Wv); ++j)
                    std::memcpy(&CT[((size_t)(r - 1) * Wv + j) * kCT], e, sizeof e);
            }
        }
    }
    // per output row: the stripes whose boundary zone (r >= 1) or non-overlapping zone contain it, in the reference's order
    std::vector<int4> YR(Hv);
    for (int y = 0; y < Hv; ++y) {
        int lo = R, hi = -1;
        for (int r = 0; r < R; ++r) {
            const bool in_b = r >= 1 && y >= span_lo[r] && y < span_hi[r];
            const bool in_n = y >= row[8 * r + 5] && y < row[8 * r + 6];
            if (in_b || in_n) {
                lo = std::min(lo, r);
                hi = std::max(hi, r);
            }
        }
        // a plain row: one stripe's non-overlapping zone and no boundary zone -- the kernel's copy path may take it
        const bool plain = lo == hi && !(lo >= 1 && y >= span_lo[lo] && y < span_hi[lo]);
        YR[y] = make_int4(lo, hi, plain ? lo : -1, 0);
    }
    if (R == 1 && C == 1) {   // one tile: the stack itself (UnstitchedVolume.cpp:553-557)
        std::fill(ST.begin(), ST.end(), 0 | (kNone << 8));
        for (int y = 0; y < Hv; ++y) YR[y] = make_int4(0, 0, 0, 0);
        row[5] = 0;
        row[6] = Hv;
        row[4] = Wv + row[1];
    }

    // one device blob for the tables, stream-ordered
    std::vector<unsigned long long> ptrs(R * C);
    for (int s = 0; s < R * C; ++s) ptrs[s] = reinterpret_cast<unsigned long long>(stacks[s]);
    auto al = [](size_t n) { return (n + 15) & ~(size_t)15; };
    const size_t oW = 0, oP = oW + al(sizeof(double) * std::max<size_t>(W.w.size(), 1)), oRC = oP + al(8 * ptrs.size()),
                 oRow = oRC + al(4 * rc.size()), oST = oRow + al(4 * row.size()), oCT = oST + al(4 * ST.size()),
                 oYR = oCT + al(4 * std::max<size_t>(CT.size(), 1)), tot = oYR + al(sizeof(int4) * YR.size());
    std::vector<unsigned char> blob(tot, 0);
    std::memcpy(blob.data() + oW, W.w.data(), sizeof(double) * W.w.size());
    std::memcpy(blob.data() + oP, ptrs.data(), 8 * ptrs.size());
    std::memcpy(blob.data() + oRC, rc.data(), 4 * rc.size());
    std::memcpy(blob.data() + oRow, row.data(), 4 * row.size());
    std::memcpy(blob.data() + oST, ST.data(), 4 * ST.size());
    if (!CT.empty()) std::memcpy(blob.data() + oCT, CT.data(), 4 * CT.size());
    std::memcpy(blob.data() + oYR, YR.data(), sizeof(int4) * YR.size());

    MI_TRY(mi::use_device(dev));
    hipStream_t s = mi::as_stream(stream);
    void* dblob = nullptr;
    MI_HIP(hipMallocAsync(&dblob, tot, s));
    // pageable source: the call returns once the bytes are staged, so the host vector may go when it returns
    hipError_t e = hipMemcpyAsync(dblob, blob.data(), tot, hipMemcpyHostToDevice, s);
    if (e != hipSuccess) {
        (void)hipFreeAsync(dblob, s);
        return mi::fail(MI_ERR_HIP, "mi_merge_slab: table upload failed: %s", hipGetErrorString(e));
    }
    const unsigned char* b = static_cast<const unsigned char*>(dblob);
    Params p;
    p.W = reinterpret_cast<const double*>(b + oW);
    p.stk = reinterpret_cast<const unsigned long long*>(b + oP);
    p.rc = reinterpret_cast<const int*>(b + oRC);
    p.row = reinterpret_cast<const int*>(b + oRow);
    p.ST = reinterpret_cast<const int*>(b + oST);
    p.CT = reinterpret_cast<const int*>(b + oCT);
    p.YR = reinterpret_cast<const int4*>(b + oYR);
    p.R = R; p.C = C; p.Hs = Hs; p.Ws = Ws; p.Wv = Wv;
    p.bytes = bytes; p.blending = blending;
    p.D0 = D0; p.V0 = V0; p.H0 = H0; p.Vb = V1 - V0; p.Hb = H1 - H0;
    p.scale = bytes == 2 ? 65535.0f : 255.0f;
    const int groups = (p.Hb + kVec - 1) / kVec;
    dim3 grid((groups + 255) / 256, p.Vb, D1 - D0);
    hipLaunchKernelGGL(merge_kernel, grid, dim3(256), 0, s, p, out);
    const int rc_launch = mi::launch_check("merge_kernel");
    (void)hipFreeAsync(dblob, s);
    return rc_launch;
}
