// The device TIFF reader (include/mi_tiffio.h, mi_tiff_read_box_device): the mirror of the device writer in tiff_deflate.hip.  The host
// parses the directories and reads the compressed strips into pinned memory; the bytes cross to the device as they are in the files,
// and two kernels make the box there:
//   k_strip_inflate         one zlib stream per wave (a work-group is one wave).  The decoder is the text of tiff_inflate_dev.h: every
//                           lane runs the serial symbol decode with the same values (what the core uses as uniform comes through
//                           readfirstlane, so the compiler keeps it in scalar registers), and the lanes part where there is width:
//                           staging the compressed bytes into LDS, filling the lookup tables, copying matches, writing the output
//                           out as words, the two sums of the Adler-32.
//   k_strip_unpredict_crop  undoes horizontal differencing (a scan per row) and copies the box's rows and columns of every strip to
//                           out[k][y - y0][x - x0].  Strips that are not compressed take this kernel alone.
//
// The history window of a stream is its own output: the last bytes (up to kPend + 258) wait in LDS until they go out to global memory
// as whole words, everything before lies in global memory.  A match reads each byte from where it is.  What orders the accesses:
//   - a lane reads LDS bytes another lane wrote (staged input, the lookup tables filled an entry per lane, pending output): a
//     __syncthreads() stands between every such write and read -- a work-group is one wave, so the barrier costs no waiting, it is
//     the fence that counts;
//   - the serial parts of the core (code lengths, build_code, the pending literal) are run by all 64 lanes with the same addresses
//     and values: every lane reads what it wrote itself, in program order; this rests on the work-group being ONE wave
//     (__launch_bounds__(64), launched with 64 threads);
//   - a lane reads global bytes another lane wrote (a match that reaches behind the pending bytes; the Adler sums): those bytes were
//     written by flush(), which ends in __syncthreads() -- a work-group release / acquire of global memory -- before `flushed` moves.
// LDS per wave: sizeof(InflateLds) = 9 340 bytes (tables 3 956, staged input 1 024, pending output 4 360): 17 waves per CU by LDS
// (160 KiB), 20 by registers (83 VGPRs: 5 waves per SIMD); a box of 64 slices of 8 strips is 512 waves, two per CU.

#include <algorithm>
#include <cerrno>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

#include "mi_internal.h"
#include "mi_tiffio.h"
#include "tiff_inflate_dev.h"
#include "tiffio_internal.h"

namespace {

using mi::fail;
using namespace mi_inflate;

constexpr int kStageWords = 256;             // compressed bytes in LDS: 1 KB at a time
constexpr int kPend = 4096;                  // output bytes that wait in LDS; flushed when this many are there
constexpr int kPendBytes = kPend + 264;      // + the alignment offset (3) + the longest match (258), a multiple of 4

struct InflateLds {
    InfTables t;
    uint32_t in[kStageWords];
    uint32_t pend[kPendBytes / 4];
};
static_assert(sizeof(InflateLds) <= 9600, "17 waves per CU: at most 160 KiB / 17 of LDS per wave");

struct StripJob {
    unsigned long long in_off, out_off;   // into the uploaded bytes / the inflated bytes; both multiples of 16
    uint32_t in_n, out_n;
};

// the context of tiff_inflate_dev.h for a wave: out[0, flushed) is in global memory, out[flushed, flushed + npend) waits in
// s.pend from byte (flushed & 3) on, so that LDS words and global words coincide
struct WaveCtx {
    InflateLds& s;
    const unsigned char* __restrict__ in;
    uint32_t in_n;
    unsigned char* out;
    uint32_t lane, stage_base, flushed, npend;

    __device__ __forceinline__ uint32_t uni(uint32_t v) const { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
    __device__ __forceinline__ InfTables& tables() { return s.t; }

    // words [first, first + kStageWords) of the stream; no byte at or beyond in_n is read
    __device__ __forceinline__ void stage(uint32_t first) {
        __syncthreads();
        stage_base = first;
        for (uint32_t k = lane; k < (uint32_t)kStageWords; k += 64) {
            const unsigned long long at = ((unsigned long long)first + k) * 4u;
            uint32_t v = 0;
            if (at + 4 <= in_n) v = *reinterpret_cast<const uint32_t*>(in + at);
            else
                for (uint32_t b = 0; b < 4; ++b)
                    if (at + b < in_n) v |= (uint32_t)in[at + b] << (8 * b);
            s.in[k] = v;
        }
        __syncthreads();
    }
    __device__ __forceinline__ uint32_t word(uint32_t i) {
        if (i - stage_base >= (uint32_t)kStageWords) stage(i);
        return uni(s.in[i - stage_base]);
    }
    template <class F>
    __device__ __forceinline__ void for_each(uint32_t n, F f) {
        __syncthreads();
        for (uint32_t i = lane; i < n; i += 64) f(i);
        __syncthreads();
    }
    __device__ __forceinline__ void flush() {
        __syncthreads();
        const unsigned char* pb = reinterpret_cast<const unsigned char*>(s.pend);
        const uint32_t off = flushed & 3u, end = off + npend;
        unsigned char* g = out + (flushed - off);
        for (uint32_t w = lane; 4 * w < end; w += 64) {
            const uint32_t lo = 4 * w, hi = lo + 4;
            if (lo >= off && hi <= end) *reinterpret_cast<uint32_t*>(g + lo) = s.pend[w];
            else
                for (uint32_t b = lo > off ? lo : off; b < (hi < end ? hi : end); ++b) g[b] = pb[b];
        }
        flushed += npend;
        npend = 0;
        __syncthreads();
    }
    __device__ __forceinline__ void literal(uint32_t, uint32_t b) {
        reinterpret_cast<unsigned char*>(s.pend)[(flushed & 3u) + npend] = (unsigned char)b;
        npend += 1;
        if (npend >= (uint32_t)kPend) flush();
    }
    // every source byte lies before pos: in the pending bytes or in global memory, never in what this match writes
    __device__ __forceinline__ void match(uint32_t pos, uint32_t dist, uint32_t len) {
        unsigned char* pb = reinterpret_cast<unsigned char*>(s.pend);
        const uint32_t off = flushed & 3u, src0 = pos - dist;
        __syncthreads();
        for (uint32_t k = lane; k < len; k += 64) {
            const uint32_t p = src0 + (dist >= len ? k : k % dist);
            pb[off + npend + k] = p >= flushed ? pb[off + (p - flushed)] : out[p];
        }
        __syncthreads();
        npend += len;
        if (npend >= (uint32_t)kPend) flush();
    }
    __device__ __forceinline__ uint32_t adler(uint32_t n) {
        flush();
        unsigned long long s1 = 0, s2 = 0;
        const uint32_t nw = n / 4;
        const uint32_t* w32 = reinterpret_cast<const uint32_t*>(out);
        uint32_t round = 0;
        for (uint32_t w = lane; w < nw; w += 64) {
            const uint32_t v = w32[w];
            for (uint32_t b = 0; b < 4; ++b) {
                const uint32_t x = (v >> (8 * b)) & 255u;
                s1 += x;
                s2 += (unsigned long long)(n - (4 * w + b)) * x;
            }
            if ((++round & 4095u) == 0) s2 %= 65521ull;
        }
        if (lane < (n & 3u)) {
            const uint32_t i = 4 * nw + lane, x = out[i];
            s1 += x;
            s2 += (unsigned long long)(n - i) * x;
        }
        s1 %= 65521ull;
        s2 %= 65521ull;
        for (int o = 32; o > 0; o >>= 1) {
            s1 += __shfl_down(s1, o, 64);
            s2 += __shfl_down(s2, o, 64);
        }
        const uint32_t a = uni((uint32_t)((1ull + s1) % 65521ull)), b = uni((uint32_t)(((unsigned long long)n + s2) % 65521ull));
        return b << 16 | a;
    }
};

__global__ __launch_bounds__(64) void k_strip_inflate(const unsigned char* __restrict__ in, unsigned char* out, const StripJob* __restrict__ jobs,
                                                      int32_t* __restrict__ status) {
    __shared__ InflateLds s;
    const StripJob j = jobs[blockIdx.x];
    const uint32_t in_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)j.in_n), out_n = (uint32_t)__builtin_amdgcn_readfirstlane((int)j.out_n);
    WaveCtx ctx{s, in + j.in_off, in_n, out + j.out_off, threadIdx.x, 0, 0, 0};
    ctx.stage(0);
    const int st = inflate_zlib(ctx, in_n, out_n);
    if (threadIdx.x == 0) status[blockIdx.x] = st;
}

struct CropJob {
    unsigned long long src_off;    // the strip's rows (inflated, or as uploaded)
    uint32_t row0, nrows, out_row; // the first row of the strip that lies in the box, how many do, and the first's row in out (k * (y1 - y0) + y - y0)
    uint32_t pred;                 // 1: the file stores differences to the left neighbour (predictor 2)
};

// a wave per row; pred: the stored samples are differences to the left neighbour, wrapping in T: an inclusive scan along the row,
// four samples per lane and step
template <class T>
__global__ __launch_bounds__(256) void k_strip_unpredict_crop(const unsigned char* __restrict__ src, const CropJob* __restrict__ jobs, T* __restrict__ out,
                                                              uint32_t nx, uint32_t x0, uint32_t x1) {
    const CropJob j = jobs[blockIdx.y];
    const bool pred = sizeof(T) < 4 && j.pred != 0;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, bw = x1 - x0;
    for (uint32_t r = blockIdx.x * 4 + wave; r < j.nrows; r += gridDim.x * 4) {
        const T* row = reinterpret_cast<const T*>(src + j.src_off) + (size_t)(j.row0 + r) * nx;
        T* dst = out + (size_t)(j.out_row + r) * bw;
        if (!pred) {
            for (uint32_t x = x0 + lane; x < x1; x += 64) dst[x - x0] = row[x];
            continue;
        }
        T carry = 0;
        for (uint32_t xb = 0; xb < x1; xb += 256) {
            const uint32_t xa = xb + 4 * lane;
            T v[4];
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q) v[q] = xa + q < x1 ? row[xa + q] : (T)0;
#pragma unroll
            for (uint32_t q = 1; q < 4; ++q) v[q] = (T)(v[q] + v[q - 1]);
            uint32_t incl = v[3];
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o, 64);
                if ((int)lane >= o) incl += up;
            }
            const T before = (T)(carry + (T)(incl - v[3]));
#pragma unroll
            for (uint32_t q = 0; q < 4; ++q)
                if (xa + q >= x0 && xa + q < x1) dst[xa + q - x0] = (T)(v[q] + before);
            carry = (T)(carry + (T)__shfl(incl, 63, 64));
        }
    }
}

// ------------------------------------------------------------------------------------------------ host
using mi::slot;

mi::ScratchPool g_scratch;   // this reader's own

struct Strip {
    int file;
    uint32_t index, row0, nrows, out_row;   // CropJob's rows
    uint64_t off;
    size_t read, want;                      // bytes to read from the file; bytes of the strip's rows
    bool packed;
};

template <class T>
void launch_crop(hipStream_t s, uint32_t max_rows, uint32_t njobs, const unsigned char* src, const CropJob* jobs, void* out, int nx, int x0, int x1) {
    const uint32_t gx = std::min<uint32_t>(1024u, (max_rows + 3) / 4);
    hipLaunchKernelGGL(k_strip_unpredict_crop<T>, dim3(gx, njobs), dim3(256), 0, s, src, jobs, static_cast<T*>(out), (uint32_t)nx, (uint32_t)x0, (uint32_t)x1);
}

}  // namespace

namespace mi {
void tiff_inflate_drop_scratch(int dev) { g_scratch.drop(dev); }
}  // namespace mi

extern "C" int mi_tiff_read_box_device(int dev, void* stream, const char* const* paths, int n, int nx, int ny, int dtype, int y0, int y1, int x0, int x1,
                                       void* out, int n_threads) {
    MI_TRY(mi::use_device(dev));
    MI_REQUIRE(paths && out, "mi_tiff_read_box_device: null pointer");
    MI_REQUIRE(n >= 0 && nx > 0 && ny > 0 && (dtype == 1 || dtype == 2 || dtype == 4), "mi_tiff_read_box_device: invalid extents or sample type");
    MI_REQUIRE(0 <= y0 && y0 < y1 && y1 <= ny && 0 <= x0 && x0 < x1 && x1 <= nx, "mi_tiff_read_box_device: box [%d, %d) x [%d, %d) outside %d x %d", y0,
               y1, x0, x1, ny, nx);
    if (n == 0) return MI_OK;
    hipStream_t s = mi::as_stream(stream);
    const size_t bps = (size_t)(dtype == 4 ? 4 : dtype), rowb = (size_t)nx * bps;

    // the directories, a file per task: the host reader's checks and words
    std::vector<mi::TiffStrips> dirs((size_t)n);
    MI_TRY(mi::run_jobs(n, mi::series_threads(n_threads, n), [&](int k, int) { return mi::tiff_strips(paths[k], nx, ny, dtype, y0, y1, dirs[(size_t)k]); }));
    std::vector<Strip> strips;
    for (int k = 0; k < n; ++k) {
        const mi::TiffStrips& d = dirs[(size_t)k];
        for (uint32_t si = (uint32_t)y0 / d.rps; si <= (uint32_t)(y1 - 1) / d.rps; ++si) {
            const uint32_t r0 = si * d.rps, r1 = std::min<uint32_t>((uint32_t)ny, r0 + d.rps);
            const uint32_t a = std::max<uint32_t>(r0, (uint32_t)y0), b = std::min<uint32_t>(r1, (uint32_t)y1);
            Strip st;
            st.file = k;
            st.index = si;
            st.row0 = a - r0;
            st.nrows = b - a;
            st.out_row = (uint32_t)k * (uint32_t)(y1 - y0) + (a - (uint32_t)y0);
            st.off = d.off[si];
            st.want = (size_t)(r1 - r0) * rowb;
            st.packed = d.comp != 1;
            st.read = st.packed ? (size_t)d.cnt[si] : st.want;
            MI_REQUIRE(st.read < 0x7fffffffull && st.want < 0x7fffffffull, "%s: strip %u is larger than the device reader takes (2 GB)", paths[k], si);
            strips.push_back(st);
        }
    }
    MI_REQUIRE((uint64_t)n * (uint64_t)(y1 - y0) < 0xffffffffull, "mi_tiff_read_box_device: more than 2^32 rows in the box");

    const std::shared_ptr<mi::DeviceScratch> sc = g_scratch.get(dev);
    std::lock_guard<std::mutex> hold(sc->mu);

    // batches of bounded size: at most 1 GB of file bytes, 1 GB of inflated rows and 16384 strips at a time.  A stream is a wave and
    // takes its time however many run beside it (a 1-MB strip: 70 - 270 ms), so a batch holds as many streams as the bounds allow:
    // the box of 64 slices of 8 MB is one batch of 512 waves
    constexpr size_t kMaxRead = (size_t)1 << 30, kMaxRows = (size_t)1 << 30, kMaxStrips = 16384;
    for (size_t b0 = 0; b0 < strips.size();) {
        size_t b1 = b0, read_bytes = 0, row_bytes = 0, n_packed = 0;
        uint32_t max_rows = 0;
        while (b1 < strips.size()) {
            const Strip& st = strips[b1];
            const size_t rb = read_bytes + slot(st.read), wb = row_bytes + (st.packed ? slot(st.want) : 0);
            if (b1 > b0 && (rb > kMaxRead || wb > kMaxRows || b1 - b0 >= kMaxStrips)) break;
            read_bytes = rb;
            row_bytes = wb;
            n_packed += st.packed ? 1 : 0;
            max_rows = std::max(max_rows, st.nrows);
            ++b1;
        }
        const size_t nb = b1 - b0;
        // the jobs: [StripJob x n_packed | CropJob x nb | status x n_packed], the same layout on both sides
        const auto [crop_at, status_at, jobs_bytes] = mi::job_layout(n_packed, sizeof(StripJob), nb, sizeof(CropJob), n_packed, sizeof(int32_t));
        MI_TRY(sc->h_bytes.reserve(read_bytes));
        MI_TRY(sc->h_jobs.reserve(jobs_bytes));
        MI_TRY(sc->grow(sc->d_bytes, read_bytes + row_bytes));   // the file's bytes, then the inflated rows
        MI_TRY(sc->grow(sc->d_jobs, jobs_bytes));
        unsigned char* hb = sc->h_bytes.as<unsigned char>();
        StripJob* sj = reinterpret_cast<StripJob*>(sc->h_jobs.as<unsigned char>());
        CropJob* cj = reinterpret_cast<CropJob*>(sc->h_jobs.as<unsigned char>() + crop_at);
        int32_t* status = reinterpret_cast<int32_t*>(sc->h_jobs.as<unsigned char>() + status_at);
        std::vector<size_t> read_at(nb), packed_strip;
        size_t ra = 0, wa = 0;
        for (size_t i = 0; i < nb; ++i) {
            const Strip& st = strips[b0 + i];
            read_at[i] = ra;
            cj[i].row0 = st.row0;
            cj[i].nrows = st.nrows;
            cj[i].out_row = st.out_row;
            cj[i].pred = dirs[(size_t)st.file].predictor == 2 ? 1u : 0u;
            cj[i].src_off = st.packed ? read_bytes + wa : ra;
            if (st.packed) {
                StripJob& q = sj[packed_strip.size()];
                q.in_off = ra;
                q.out_off = wa;
                q.in_n = (uint32_t)st.read;
                q.out_n = (uint32_t)st.want;
                status[packed_strip.size()] = -1;
                packed_strip.push_back(b0 + i);
                wa += slot(st.want);
            }
            ra += slot(st.read);
        }
        MI_TRY(mi::run_jobs((int)nb, mi::series_threads(n_threads, (int)nb), [&](int i, int) -> std::string {
            const Strip& st = strips[b0 + (size_t)i];
            const char* path = paths[st.file];
            mi::Fd f(path);
            if (f.fd < 0) return std::string(path) + ": " + std::strerror(errno);
            return mi::pread_all(f.fd, hb + read_at[(size_t)i], st.read, st.off) ? std::string() : std::string(path) + ": " + mi::kTruncatedStrip;
        }));
        unsigned char* d_all = sc->d_bytes.as<unsigned char>();
        unsigned char* dj = sc->d_jobs.as<unsigned char>();
        MI_HIP(hipMemcpyAsync(d_all, hb, read_bytes, hipMemcpyHostToDevice, s));
        MI_HIP(hipMemcpyAsync(dj, sc->h_jobs.p, jobs_bytes, hipMemcpyHostToDevice, s));
        if (n_packed) {
            hipLaunchKernelGGL(k_strip_inflate, dim3((uint32_t)n_packed), dim3(64), 0, s, d_all, d_all + read_bytes, reinterpret_cast<const StripJob*>(dj),
                               reinterpret_cast<int32_t*>(dj + status_at));
            MI_TRY(mi::launch_check("k_strip_inflate"));
            MI_HIP(hipMemcpyAsync(status, dj + status_at, n_packed * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        }
        const CropJob* d_cj = reinterpret_cast<const CropJob*>(dj + crop_at);
        if (bps == 1) launch_crop<uint8_t>(s, max_rows, (uint32_t)nb, d_all, d_cj, out, nx, x0, x1);
        else if (bps == 2) launch_crop<uint16_t>(s, max_rows, (uint32_t)nb, d_all, d_cj, out, nx, x0, x1);
        else launch_crop<uint32_t>(s, max_rows, (uint32_t)nb, d_all, d_cj, out, nx, x0, x1);
        MI_TRY(mi::launch_check("k_strip_unpredict_crop"));
        MI_HIP(hipStreamSynchronize(s));
        for (size_t q = 0; q < n_packed; ++q) {
            if (status[q] == kInfOk) continue;
            const Strip& st = strips[packed_strip[q]];
            return fail(MI_ERR_INVALID, "%s: strip %u does not inflate to its rows (status %d: %s)", paths[st.file], st.index, (int)status[q],
                        status_name(status[q]));
        }
        b0 = b1;
    }
    return MI_OK;
}
