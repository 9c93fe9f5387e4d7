// The one internal header of the TIFF units: tiffio.hip (the slice series on the host), tiff_deflate.hip and tiff_inflate.hip (its
// writer and reader on the device), tiff3d.hip and tiff3d_read.hip (the block files of the TeraFly tree).  What more than one of them
// needs is defined here once: the small file helpers, the two thread policies, the strip-rows rule, the tail of a slice file, the
// checks a slice passes before one of its strips is read, and the scratch and job-list layout of the device readers.  Not part of
// the C ABI.
#pragma once
#include <fcntl.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mi_internal.h"

namespace mi {

// ------------------------------------------------------------------------------------------------ files and bytes
struct Fd {
    int fd;
    explicit Fd(const char* p) : fd(open(p, O_RDONLY | O_CLOEXEC)) {}
    ~Fd() {
        if (fd >= 0) close(fd);
    }
};

inline bool pread_all(int fd, void* buf, size_t n, uint64_t at) {
    char* p = static_cast<char*>(buf);
    while (n) {
        const ssize_t r = pread(fd, p, n, (off_t)at);
        if (r <= 0) {
            if (r < 0 && errno == EINTR) continue;
            return false;
        }
        p += r;
        at += (uint64_t)r;
        n -= (size_t)r;
    }
    return true;
}

inline bool write_all(int fd, const void* buf, size_t n) {
    const char* p = static_cast<const char*>(buf);
    while (n) {
        const ssize_t r = write(fd, p, n);
        if (r <= 0) {
            if (r < 0 && errno == EINTR) continue;
            return false;
        }
        p += r;
        n -= (size_t)r;
    }
    return true;
}

// little-endian
inline void put16(std::vector<unsigned char>& b, uint32_t v) { b.push_back((unsigned char)(v & 255)); b.push_back((unsigned char)(v >> 8 & 255)); }
inline void put32(std::vector<unsigned char>& b, uint32_t v) { put16(b, v & 0xffff); put16(b, v >> 16); }
inline void put64(std::vector<unsigned char>& b, uint64_t v) { put32(b, (uint32_t)v); put32(b, (uint32_t)(v >> 32)); }

// ------------------------------------------------------------------------------------------------ threads
// the cores this process may keep busy: its affinity mask capped by the cgroup CPU quota (tiffio.hip)
int host_cores();

// The slice series' policy: the threads of a call that was asked for `asked` (<= 0: all cores) and has `jobs` tasks.
inline int series_threads(int asked, int jobs) { return std::max(1, std::min(asked > 0 ? asked : host_cores(), jobs)); }

// The tree's policy: the pool of a call that was asked for n_threads (<= 0: OMP_NUM_THREADS, else 16); the caller caps it by its tasks.
inline int tree_pool_threads(int n_threads) {
    if (n_threads > 0) return n_threads;
    if (const char* e = std::getenv("OMP_NUM_THREADS")) {
        const int v = std::atoi(e);
        if (v > 0) return v;
    }
    return 16;   // never the machine's core count: a GPU host shares its cores between jobs
}

// runs job(k, thread) for k < jobs on nt threads; the first error message wins
template <class F>
int run_jobs(int jobs, int nt, F&& job) {
    std::atomic<int> next{0};
    std::mutex mu;
    std::string err;
    auto worker = [&](int t) {
        for (;;) {
            const int k = next.fetch_add(1);
            if (k >= jobs) return;
            {
                std::lock_guard<std::mutex> g(mu);
                if (!err.empty()) return;
            }
            std::string e = job(k, t);
            if (!e.empty()) {
                std::lock_guard<std::mutex> g(mu);
                if (err.empty()) err = std::move(e);
                return;
            }
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(worker, t);
    worker(0);
    for (auto& x : th) x.join();
    if (!err.empty()) return fail(MI_ERR_INVALID, "%s", err.c_str());
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------ the slice series' files
// Strips of ~1 MiB of rows: a reader that wants a few rows inflates a few strips.  The rows per strip of a slice of ny rows of rowb bytes.
inline uint32_t strip_rows_per_strip(size_t ny, size_t rowb) {
    return (uint32_t)std::max<size_t>(1, std::min<size_t>(ny, ((size_t)1 << 20) / std::max<size_t>(1, rowb)));
}

struct TiffEntry { uint16_t tag, type; uint32_t count, value; };
// three SHORTs of value v, which do not fit their entry: they lie in front of the directory and the entry of `tag` gets their place as its value
struct TiffTriple { uint16_t tag; uint32_t v; };

// The tail of a slice file whose header room (8 bytes) and strips (off, cnt) are in `file`: strip tables (when there is more than one
// strip) | triples | directory, then the header; written under a temporary name and renamed.  `ents` in tag order; the entries 273
// and 279 get their count and value here.  "" or the message.  (tiffio.hip)
std::string finish_file(const char* path, std::vector<unsigned char>& file, const std::vector<uint32_t>& off, const std::vector<uint32_t>& cnt,
                        std::vector<TiffEntry> ents, const std::vector<TiffTriple>& triples = {});
// the directory of a slice of one sample per pixel; tag 317 is left out when nothing is predicted (predictor 1)  (tiffio.hip)
std::vector<TiffEntry> gray_entries(int nx, int ny, int dtype, int compression, uint32_t rps, int predictor);

struct TiffStrips {
    uint32_t rps = 0, comp = 1, predictor = 1;
    std::vector<uint64_t> off, cnt;   // of every strip of the file
};

// Opens the file and puts it through the checks of mi_tiff_read_box's read_slice (tiffio.hip, checked_strips -- the very function
// read_slice calls): parsed, fast, of the first slice's extents and type, the strips that rows [y0, y1) touch inside the file (raw
// strips: as long as their rows).  "" or the host reader's message.
std::string tiff_strips(const char* path, int nx, int ny, int dtype, int y0, int y1, TiffStrips& out);

// what every reader says after the path when a strip that lies inside the file cannot be read whole
constexpr const char* kTruncatedStrip = "truncated strip";

// ------------------------------------------------------------------------------------------------ the tree's block files
// What the host writer (tiff3d.hip) and the device route (tiff3d_lzw_enc.hip) share: the block walk and the page and directory
// assembly.  Both routes hand the same function their strips, so the files differ only where the streams do.
struct StripRef {
    const unsigned char* p;   // the strip as it goes into the file (encoded or raw)
    size_t n;
};

struct Tiff3dBlock {
    std::string path;
    const uint8_t* first;   // sample (0, 0, 0) of the block; host or device memory, the route knows which
    int64_t sp, sr;         // page / row strides in samples
    int w, h, pages, page0, total;
    int64_t strip0;         // index of its first strip in the list of all strips: (block, page, strip) order
};

// the arguments of mi_tiff3d_write_blocks checked and turned into blocks (first may be NULL: no samples, the strips are given); `who` begins the messages
int tiff3d_parse_blocks(const char* who, int n, const char* const* paths, const void* const* first, const int64_t* strides, const int* dims,
                        const int* page0, const int* page_total, int bytes, int rows_per_strip, std::vector<Tiff3dBlock>& blocks, int64_t* n_strips);
// every block gets its pages appended, files in parallel on `threads` threads; strips[B.strip0 + page * strips per page + strip]
int tiff3d_write_files(const std::vector<Tiff3dBlock>& blocks, const StripRef* strips, int bytes, int compression, int rows_per_strip, int bigtiff,
                       int threads);

// ------------------------------------------------------------------------------------------------ the device readers
// parts of a buffer begin at multiples of 16 bytes
inline size_t slot(size_t n) { return (n + 15) & ~(size_t)15; }

// The job lists of a batch, the same layout in pinned and in device memory: [jobs A | jobs B | status], each part from a multiple of 16.
struct JobLayout {
    size_t b_at, status_at, bytes;
};
inline JobLayout job_layout(size_t n_a, size_t size_a, size_t n_b, size_t size_b, size_t n_status, size_t size_status) {
    const size_t b_at = slot(n_a * size_a), status_at = b_at + slot(n_b * size_b);
    return {b_at, status_at, status_at + slot(n_status * size_status)};
}

// The scratch of a device: pinned and device memory sized by the largest batch seen, kept between calls and given back by
// mi_release_cached_memory.  A call holds `mu` from its first batch to its last.
struct DeviceScratch {
    std::mutex mu;
    PinnedBuf h_bytes, h_jobs;
    DevBuf d_bytes, d_jobs;
    static int grow(DevBuf& b, size_t n) { return n <= b.bytes ? MI_OK : b.alloc(n + n / 8); }
};

// One reader's scratches, a device each.  Every reader has a pool of its own: the readers neither share memory nor wait for each other.
class ScratchPool {
    std::mutex mu_;
    std::map<int, std::shared_ptr<DeviceScratch>>& of_ = *new std::map<int, std::shared_ptr<DeviceScratch>>;   // (never destroyed: the runtime may be gone by then)

  public:
    std::shared_ptr<DeviceScratch> get(int dev) {
        std::lock_guard<std::mutex> g(mu_);
        std::shared_ptr<DeviceScratch>& e = of_[dev];
        if (!e) e = std::make_shared<DeviceScratch>();
        return e;
    }
    // dev < 0: of every device
    void drop(int dev) {
        std::lock_guard<std::mutex> g(mu_);
        for (auto it = of_.begin(); it != of_.end();) {
            if (dev < 0 || it->first == dev) it = of_.erase(it);   // (a call in flight keeps its scratch until it returns)
            else ++it;
        }
    }
};

}  // namespace mi
