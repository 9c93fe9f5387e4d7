// What tiffio.hip shares with the device reader (tiff_inflate.hip): the checks a file passes before one of its strips is read, so
// that both readers take the same files and refuse the others in the same words, and the small host helpers of both.  Not part of
// the C ABI.
#pragma once
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <cstdint>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mi_internal.h"

namespace mi {

struct TiffStrips {
    uint32_t rps = 0, comp = 1, predictor = 1;
    std::vector<uint64_t> off, cnt;   // of every strip of the file
};

// Opens the file and puts it through the checks of mi_tiff_read_box's read_slice (tiffio.hip, checked_strips -- the very function
// read_slice calls): parsed, fast, of the first slice's extents and type, the strips that rows [y0, y1) touch inside the file (raw
// strips: as long as their rows).  "" or the host reader's message.
std::string tiff_strips(const char* path, int nx, int ny, int dtype, int y0, int y1, TiffStrips& out);

// the threads of a call that was asked for `asked` (<= 0: all cores) and has `jobs` tasks
int tiff_thread_count(int asked, int jobs);

// what both readers say after the path when a strip that lies inside the file cannot be read whole
constexpr const char* kTruncatedStrip = "truncated strip";

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

}  // namespace mi
