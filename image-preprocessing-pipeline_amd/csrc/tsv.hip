// The live tile merge of the pipeline (include/mi_tsv.h): a box of a TSVVolume, `maximum` or the float16 cosine blend.
//
// The host cuts the box's XY plane into the cells of the sorted stack edges: within a cell the list of covering stacks is
// constant (row-major order, the order of the blend).  A work-group works on a piece of ONE cell, so the list, the pair
// parameters and every branch on them are uniform over the group; only the z test of a stack depends on the plane, and the
// plane is the group's too.  Lanes run along x, each makes kVec consecutive output samples; the lanes' runs are laid on the
// 16-byte grid of the output ROW (rows of an odd-width box shift against each other), so every run that lies wholly in the cell
// is one vector store.  Stack rows start anywhere: a run is read as one vector, as dwords or sample by sample, as its address
// allows.  All offsets are 64-bit.
//
// Cosine blend (tsv/volume.py:592-631): with all stacks of one shape and no two at the same (x0, y0), get_distance_from_edge
// (:490-555) never takes its inf / z branches, and the edge distance of a stack inside its overlap with another is
//     d = min(max_distance, [XMIN] x - ox0 + 1, [XMAX] ox1 - x, [YMIN] y - oy0 + 1, [YMAX] oy1 - y)
// over the pair's XY overlap [ox0,ox1) x [oy0,oy1): a function of the absolute position and the pair alone, whatever box was
// asked for.  The reference takes the minimum of a float32 constant and int64 ramps, which numpy makes float64, so its weight is
// float16(sin(arctan2(d, od))^2) from float64.  Here it is d^2 / (d^2 + od^2) in double (the squares and their sum are exact, the
// division correctly rounded: no fast-math) rounded ONCE to float16 -- through a float rounded to odd, so that the second rounding
// cannot double-round.  Measured on the CPU: equal to the reference's float16 weight for every d, od <= 1024.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <limits>
#include <vector>

#include "mi_internal.h"
#include "mi_tsv.h"

namespace {

constexpr int kVec = 8;          // output samples per lane
constexpr int kThreads = 256;
constexpr int kMinLanesX = 8;    // a group is lanes_x x (256 / lanes_x) lanes; lanes_x by the cell's width
enum { kXMin = 1, kXMax = 2, kYMin = 4, kYMax = 8 };   // Edge flags (tsv/volume.py:468-487)

struct StackRec { unsigned long long ptr; int x0, y0, zlo, zhi; };       // zlo / zhi: the stack's planes within the box
struct CellRec { int x0, x1, y0, y1, n, list, pairs, lanes_log2; };      // box-relative; list / pairs: first entries
struct PairRec { int ox0, ox1, oy0, oy1, maxd, fd, fod, pad; };          // absolute overlap of (stack, other stack)
struct Item { int cell, px, py, pad; };

struct Params {
    const StackRec* stacks;
    const CellRec* cells;
    const int* lists;
    const PairRec* pairs;
    const Item* items;
    int H, W;                    // stack planes
    int bx0, by0, bz0;           // box origin
    int Hb, Wb;                  // box rows, columns
    int out_aligned;             // the output's first sample lies on a 16-byte address
};

__device__ __forceinline__ float h16(float v) { return (float)(_Float16)v; }   // round to nearest-even float16

// double in (0, 1] -> float16, one rounding to nearest-even: float by round-to-odd (truncate, then set the last bit when inexact)
// keeps enough of what was cut off for the float -> float16 rounding to decide as it would on the double
__device__ __forceinline__ float weight16(double w) {
    float f = (float)w;
    unsigned bits = __float_as_uint(f);
    if ((double)f > w) --bits;                       // w > 0: the float below is the truncation
    if ((double)__uint_as_float(bits) != w) bits |= 1u;
    return h16(__uint_as_float(bits));
}

// kVec samples of a stack row from an arbitrary address; only [k0, k1) are read
template <typename T>
__device__ __forceinline__ void load_run(const T* p, int k0, int k1, unsigned* q) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (k0 == 0 && k1 == kVec && (a & 3) == 0) {
        constexpr int nw = kVec * sizeof(T) / 4;
        unsigned w[nw];
        if ((a & (kVec * sizeof(T) - 1)) == 0) {
            if constexpr (sizeof(T) == 2) {
                const uint4 v = *reinterpret_cast<const uint4*>(p);
                w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
            } else {
                const uint2 v = *reinterpret_cast<const uint2*>(p);
                w[0] = v.x; w[1] = v.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < nw; ++i) w[i] = reinterpret_cast<const unsigned*>(p)[i];
        }
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            if constexpr (sizeof(T) == 2) q[k] = (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
            else q[k] = (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < kVec; ++k) q[k] = (k >= k0 && k < k1) ? (unsigned)p[k] : 0u;
}

__device__ __forceinline__ int edge_distance(const PairRec& P, int flags, int X, int Y) {
    int d = P.maxd;
    if (flags & kXMin) d = min(d, X - P.ox0 + 1);
    if (flags & kXMax) d = min(d, P.ox1 - X);
    if (flags & kYMin) d = min(d, Y - P.oy0 + 1);
    if (flags & kYMax) d = min(d, P.oy1 - Y);
    return d;
}

template <typename T, bool kCosine>
__global__ void __launch_bounds__(kThreads) tsv_merge_kernel(Params p, T* __restrict__ out) {
#pragma clang fp contract(off)
    const Item it = p.items[blockIdx.x];
    const CellRec c = p.cells[it.cell];
    const int z = blockIdx.y;                                  // box-relative plane
    const int lanes_x = 1 << c.lanes_log2;
    const int lx = threadIdx.x & (lanes_x - 1), ly = threadIdx.x >> c.lanes_log2;
    const int y = c.y0 + it.py * (kThreads >> c.lanes_log2) + ly;
    if (y >= c.y1) return;
    const long long row = ((long long)z * p.Hb + y) * p.Wb;    // first sample of the output row
    const int xs = c.x0 + it.px * lanes_x * kVec;
    const int shift = p.out_aligned ? (int)((row + xs) & (kVec - 1)) : 0;
    const int x = xs - shift + lx * kVec;                      // this lane's run [x, x + kVec), on the row's 16-byte grid
    const int k0 = max(0, c.x0 - x), k1 = min(kVec, c.x1 - x);
    if (k0 >= k1) return;
    const int Z = p.bz0 + z, Y = p.by0 + y, X = p.bx0 + x;

    unsigned r[kVec];
    if (!kCosine) {
#pragma unroll
        for (int k = 0; k < kVec; ++k) r[k] = 0u;
        for (int i = 0; i < c.n; ++i) {
            const StackRec s = p.stacks[p.lists[c.list + i]];
            if (Z < s.zlo || Z >= s.zhi) continue;
            const T* src = reinterpret_cast<const T*>(s.ptr) + (((long long)(Z - s.zlo) * p.H + (Y - s.y0)) * p.W + (X - s.x0));
            unsigned q[kVec];
            load_run(src, k0, k1, q);
#pragma unroll
            for (int k = 0; k < kVec; ++k) r[k] = max(r[k], q[k]);
        }
    } else {
        float res[kVec], mul[kVec];
#pragma unroll
        for (int k = 0; k < kVec; ++k) res[k] = mul[k] = 0.0f;
        for (int i = 0; i < c.n; ++i) {
            const StackRec s = p.stacks[p.lists[c.list + i]];
            if (Z < s.zlo || Z >= s.zhi) continue;
            const T* src = reinterpret_cast<const T*>(s.ptr) + (((long long)(Z - s.zlo) * p.H + (Y - s.y0)) * p.W + (X - s.x0));
            unsigned q[kVec];
            load_run(src, k0, k1, q);
            float part[kVec], m[kVec];
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                part[k] = h16((float)q[k]);
                m[k] = 1.0f;
            }
            for (int j = 0; j < c.n; ++j) {
                if (j == i) continue;
                const StackRec o = p.stacks[p.lists[c.list + j]];
                if (Z < o.zlo || Z >= o.zhi) continue;
                const PairRec P = p.pairs[c.pairs + i * c.n + j];
#pragma unroll
                for (int k = 0; k < kVec; ++k) {
                    const double d = (double)edge_distance(P, P.fd, X + k, Y), od = (double)edge_distance(P, P.fod, X + k, Y);
                    const double dd = d * d, oo = od * od;
                    const float w = weight16(dd / (dd + oo));
                    part[k] = h16(part[k] * w);
                    m[k] = h16(m[k] * w);
                }
            }
#pragma unroll
            for (int k = 0; k < kVec; ++k) {
                res[k] = h16(res[k] + part[k]);
                mul[k] = h16(mul[k] + m[k]);
            }
        }
        constexpr float eps16 = 0.0009765625f;                 // finfo(float16).eps
        constexpr float top = sizeof(T) == 2 ? 65535.0f : 255.0f;
#pragma unroll
        for (int k = 0; k < kVec; ++k) {
            const float v = h16(res[k] / (mul[k] > eps16 ? mul[k] : eps16));
            r[k] = v < top ? (unsigned)v : (unsigned)top;      // inf, nan and the uint8 clip; the cast truncates
        }
    }

    T* o = out + row + x;
    if (k0 == 0 && k1 == kVec && p.out_aligned) {
        if constexpr (sizeof(T) == 2) {
            uint4 w;
            w.x = r[0] | (r[1] << 16);
            w.y = r[2] | (r[3] << 16);
            w.z = r[4] | (r[5] << 16);
            w.w = r[6] | (r[7] << 16);
            *reinterpret_cast<uint4*>(o) = w;
        } else {
            uint2 w;
            w.x = r[0] | (r[1] << 8) | (r[2] << 16) | (r[3] << 24);
            w.y = r[4] | (r[5] << 8) | (r[6] << 16) | (r[7] << 24);
            *reinterpret_cast<uint2*>(o) = w;
        }
    } else {
        for (int k = k0; k < k1; ++k) o[k] = (T)r[k];
    }
}

}  // namespace

extern "C" int mi_tsv_place(int R, int C, const int* north, const int* west, int ignore_z, const int* nz, int height, int width,
                            int* x0, int* y0, int* z0, int* extent) {
    MI_REQUIRE(R > 0 && C > 0 && north && west && nz && x0 && y0 && z0 && extent && height > 0 && width > 0,
               "mi_tsv_place: bad arguments");
    // make_stacks (tsv/volume.py:743-771): rows > 0 chain on the north neighbour, row 0 on the west one
    x0[0] = y0[0] = z0[0] = 0;
    for (int r = 0; r < R; ++r)
        for (int c = 0; c < C; ++c) {
            const int s = r * C + c;
            if (r == 0 && c == 0) continue;
            const int prev = r > 0 ? s - C : s - 1;
            const int* d = (r > 0 ? north : west) + 3 * s;
            x0[s] = x0[prev] - d[0];
            y0[s] = y0[prev] - d[1];
            z0[s] = z0[prev] - (ignore_z ? 0 : d[2]);
        }
    int mx = x0[0], my = y0[0], mz = z0[0];
    for (int s = 1; s < R * C; ++s) {
        mx = std::min(mx, x0[s]);
        my = std::min(my, y0[s]);
        mz = std::min(mz, z0[s]);
    }
    int e[6] = {std::numeric_limits<int>::max(), 0, std::numeric_limits<int>::max(), 0, std::numeric_limits<int>::max(), 0};
    for (int s = 0; s < R * C; ++s) {
        MI_REQUIRE(nz[s] >= 0, "mi_tsv_place: stack %d has %d slices", s, nz[s]);
        x0[s] -= mx;
        y0[s] -= my;
        z0[s] -= mz;
        e[0] = std::min(e[0], x0[s]);
        e[1] = std::max(e[1], x0[s] + width);
        e[2] = std::min(e[2], y0[s]);
        e[3] = std::max(e[3], y0[s] + height);
        e[4] = std::min(e[4], z0[s]);
        e[5] = std::max(e[5], z0[s] + nz[s]);
    }
    std::memcpy(extent, e, sizeof e);
    return MI_OK;
}

extern "C" int mi_tsv_merge(int dev, void* stream, int n, const int* x0, const int* y0, const int* z0, const int* nz, int H, int W,
                            const void* const* slices, int bytes, int cosine, int bx0, int bx1, int by0, int by1, int bz0, int bz1,
                            void* out) {
    MI_REQUIRE(n > 0 && x0 && y0 && z0 && nz && slices && out, "mi_tsv_merge: bad arguments");
    MI_REQUIRE(H > 0 && W > 0, "mi_tsv_merge: stacks of %d x %d", H, W);
    MI_REQUIRE(bytes == 1 || bytes == 2, "mi_tsv_merge: %d bytes per sample (1 or 2)", bytes);
    MI_REQUIRE(cosine == 0 || cosine == 1, "mi_tsv_merge: cosine %d (0 or 1)", cosine);
    MI_REQUIRE(bx0 < bx1 && by0 < by1 && bz0 < bz1, "mi_tsv_merge: empty box [%d,%d) x [%d,%d) x [%d,%d)", bx0, bx1, by0, by1, bz0, bz1);
    MI_REQUIRE(bz1 - (long long)bz0 <= 65535, "mi_tsv_merge: box of %lld planes (at most 65535)", bz1 - (long long)bz0);
    const long long lim = 1 << 30;
    MI_REQUIRE(bx0 > -lim && bx1 < lim && by0 > -lim && by1 < lim && bz0 > -lim && bz1 < lim, "mi_tsv_merge: box out of range");
    for (int s = 0; s < n; ++s)
        MI_REQUIRE(x0[s] > -lim && x0[s] < lim && y0[s] > -lim && y0[s] < lim && z0[s] > -lim && z0[s] < lim && nz[s] >= 0 && nz[s] < lim,
                   "mi_tsv_merge: stack %d out of range", s);
    const int Wb = bx1 - bx0, Hb = by1 - by0, Db = bz1 - bz0;

    // the stacks that meet the box, in the given order
    std::vector<StackRec> stacks;
    std::vector<int> ids;
    for (int s = 0; s < n; ++s) {
        const int zlo = std::max(z0[s], bz0), zhi = std::min(z0[s] + nz[s], bz1);
        if (zlo >= zhi || x0[s] >= bx1 || x0[s] + W <= bx0 || y0[s] >= by1 || y0[s] + H <= by0) continue;
        MI_REQUIRE(slices[s], "mi_tsv_merge: stack %d meets the box and has no samples", s);
        stacks.push_back(StackRec{reinterpret_cast<unsigned long long>(slices[s]), x0[s], y0[s], zlo, zhi});
        ids.push_back(s);
    }
    const int m = (int)stacks.size();
    if (cosine)
        for (int a = 0; a < m; ++a)
            for (int b = a + 1; b < m; ++b)
                MI_REQUIRE(stacks[a].x0 != stacks[b].x0 || stacks[a].y0 != stacks[b].y0,
                           "mi_tsv_merge: stacks %d and %d lie on the same XY rectangle (x0 %d, y0 %d): their cosine weights depend "
                           "on the requested box in the reference and are not built", ids[a], ids[b], stacks[a].x0, stacks[a].y0);

    // cells of the sorted edges (absolute coordinates, clipped to the box)
    std::vector<int> xe{bx0, bx1}, ye{by0, by1};
    for (const StackRec& s : stacks) {
        for (int e : {s.x0, s.x0 + W})
            if (e > bx0 && e < bx1) xe.push_back(e);
        for (int e : {s.y0, s.y0 + H})
            if (e > by0 && e < by1) ye.push_back(e);
    }
    std::sort(xe.begin(), xe.end());
    xe.erase(std::unique(xe.begin(), xe.end()), xe.end());
    std::sort(ye.begin(), ye.end());
    ye.erase(std::unique(ye.begin(), ye.end()), ye.end());

    std::vector<CellRec> cells;
    std::vector<int> lists;
    std::vector<PairRec> pairs;
    std::vector<Item> items;
    std::vector<int> in_row;
    for (size_t yi = 0; yi + 1 < ye.size(); ++yi) {
        in_row.clear();
        for (int s = 0; s < m; ++s)
            if (stacks[s].y0 <= ye[yi] && ye[yi + 1] <= stacks[s].y0 + H) in_row.push_back(s);
        for (size_t xi = 0; xi + 1 < xe.size(); ++xi) {
            CellRec c;
            c.x0 = xe[xi] - bx0; c.x1 = xe[xi + 1] - bx0; c.y0 = ye[yi] - by0; c.y1 = ye[yi + 1] - by0;
            c.list = (int)lists.size();
            for (int s : in_row)
                if (stacks[s].x0 <= xe[xi] && xe[xi + 1] <= stacks[s].x0 + W) lists.push_back(s);
            c.n = (int)lists.size() - c.list;
            c.pairs = (int)pairs.size();
            if (cosine && c.n > 1) {
                for (int i = 0; i < c.n; ++i)
                    for (int j = 0; j < c.n; ++j) {
                        PairRec P{};
                        if (i != j) {
                            const StackRec& a = stacks[lists[c.list + i]];
                            const StackRec& b = stacks[lists[c.list + j]];
                            P.ox0 = std::max(a.x0, b.x0); P.ox1 = std::min(a.x0, b.x0) + W;
                            P.oy0 = std::max(a.y0, b.y0); P.oy1 = std::min(a.y0, b.y0) + H;
                            // max_distance (:517-521): the overlap's width when the x edges differ, its height when the y edges do
                            P.maxd = std::numeric_limits<int>::max();
                            if (a.x0 != b.x0) P.maxd = P.ox1 - P.ox0;
                            if (a.y0 != b.y0) P.maxd = std::min(P.maxd, P.oy1 - P.oy0);
                            // edges (:503-511) of a against b, and of b against a
                            auto flags = [&](const StackRec& s, const StackRec& o) {
                                int f = 0;
                                if (o.x0 + W > s.x0 && s.x0 > o.x0) f |= kXMin;
                                if (o.x0 < s.x0 + W && s.x0 + W < o.x0 + W) f |= kXMax;
                                if (o.y0 + H > s.y0 && s.y0 > o.y0) f |= kYMin;
                                if (o.y0 < s.y0 + H && s.y0 + H < o.y0 + H) f |= kYMax;
                                return f;
                            };
                            P.fd = flags(a, b);
                            P.fod = flags(b, a);
                        }
                        pairs.push_back(P);
                    }
            }
            // lanes along x: the cell's width plus the worst shift to the output's 16-byte grid, in runs of kVec
            const int runs = (c.x1 - c.x0 + kVec - 1 + kVec - 1) / kVec;
            int lg = 3;
            while ((1 << lg) < runs && (1 << lg) < kThreads) ++lg;
            static_assert((1 << 3) == kMinLanesX, "lanes_x starts at kMinLanesX");
            c.lanes_log2 = lg;
            const int piece_x = (1 << lg) * kVec, piece_y = kThreads >> lg;
            const int npx = (c.x1 - c.x0 + kVec - 1 + piece_x - 1) / piece_x, npy = (c.y1 - c.y0 + piece_y - 1) / piece_y;
            const int ci = (int)cells.size();
            cells.push_back(c);
            for (int py = 0; py < npy; ++py)
                for (int px = 0; px < npx; ++px) items.push_back(Item{ci, px, py, 0});
        }
    }
    MI_REQUIRE(items.size() < (size_t)std::numeric_limits<int>::max(), "mi_tsv_merge: %zu work items", items.size());

    // one device blob for the tables, stream-ordered
    auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t oS = 0, oC = oS + al(sizeof(StackRec) * std::max<size_t>(stacks.size(), 1)), oL = oC + al(sizeof(CellRec) * cells.size()),
                 oP = oL + al(4 * std::max<size_t>(lists.size(), 1)), oI = oP + al(sizeof(PairRec) * std::max<size_t>(pairs.size(), 1)),
                 tot = oI + al(sizeof(Item) * items.size());
    std::vector<unsigned char> blob(tot, 0);
    if (!stacks.empty()) std::memcpy(blob.data() + oS, stacks.data(), sizeof(StackRec) * stacks.size());
    std::memcpy(blob.data() + oC, cells.data(), sizeof(CellRec) * cells.size());
    if (!lists.empty()) std::memcpy(blob.data() + oL, lists.data(), 4 * lists.size());
    if (!pairs.empty()) std::memcpy(blob.data() + oP, pairs.data(), sizeof(PairRec) * pairs.size());
    std::memcpy(blob.data() + oI, items.data(), sizeof(Item) * items.size());

    MI_TRY(mi::use_device(dev));
    hipStream_t st = mi::as_stream(stream);
    void* dblob = nullptr;
    MI_HIP(hipMallocAsync(&dblob, tot, st));
    // pageable source: the call returns once the bytes are staged, so the host vector may go when it returns
    hipError_t e = hipMemcpyAsync(dblob, blob.data(), tot, hipMemcpyHostToDevice, st);
    if (e != hipSuccess) {
        (void)hipFreeAsync(dblob, st);
        return mi::fail(MI_ERR_HIP, "mi_tsv_merge: table upload failed: %s", hipGetErrorString(e));
    }
    const unsigned char* b = static_cast<const unsigned char*>(dblob);
    Params p;
    p.stacks = reinterpret_cast<const StackRec*>(b + oS);
    p.cells = reinterpret_cast<const CellRec*>(b + oC);
    p.lists = reinterpret_cast<const int*>(b + oL);
    p.pairs = reinterpret_cast<const PairRec*>(b + oP);
    p.items = reinterpret_cast<const Item*>(b + oI);
    p.H = H; p.W = W;
    p.bx0 = bx0; p.by0 = by0; p.bz0 = bz0;
    p.Hb = Hb; p.Wb = Wb;
    p.out_aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const dim3 grid((unsigned)items.size(), (unsigned)Db);
    if (bytes == 2) {
        if (cosine) hipLaunchKernelGGL((tsv_merge_kernel<uint16_t, true>), grid, dim3(kThreads), 0, st, p, static_cast<uint16_t*>(out));
        else hipLaunchKernelGGL((tsv_merge_kernel<uint16_t, false>), grid, dim3(kThreads), 0, st, p, static_cast<uint16_t*>(out));
    } else {
        if (cosine) hipLaunchKernelGGL((tsv_merge_kernel<uint8_t, true>), grid, dim3(kThreads), 0, st, p, static_cast<uint8_t*>(out));
        else hipLaunchKernelGGL((tsv_merge_kernel<uint8_t, false>), grid, dim3(kThreads), 0, st, p, static_cast<uint8_t*>(out));
    }
    const int rc = mi::launch_check("tsv_merge_kernel");
    (void)hipFreeAsync(dblob, st);
    return rc;
}
