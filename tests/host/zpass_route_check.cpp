// Host check of z_full_grid (csrc/fft_native_route.h), compiled with g++ by tests/test_zpass_route_host.py: the paired z pass drops its
// plane bounds exactly when every z plane of the grid is read and written and MI_FFT_Z_GENERAL is not set.  Prints one line per
// failure; exit status = number of failures.
#include <cstdio>

#include "fft_native_route.h"

using namespace mi;

static int failures = 0;
static void expect(bool got, bool want, const char* what) {
    if (got != want) {
        std::printf("FAIL %s: got %d, want %d\n", what, (int)got, (int)want);
        ++failures;
    }
}

int main() {
    int checked = 0;
    // paired grids (x, y, z): the benchmark's, the smallest paired one, a radix-3 z and a 16-wave z
    const int grids[][3] = {{2048, 2048, 512}, {32, 16, 64}, {128, 64, 192}, {64, 32, 768}, {64, 16, 1024}};
    for (const auto& F : grids) {
        NativeSwitches sw;
        NativeDims d{};
        NativeSizes sz{};
        if (plan_geometry(F, sw, &d, &sz) != 0 || !d.paired) {
            std::printf("FAIL grid %d x %d x %d is not a paired plan\n", F[0], F[1], F[2]);
            return 100;
        }
        expect(z_full_grid(d, sw), true, "full grid");
        NativeDims e = d;
        e.z_in_hi = d.nz - 1;
        expect(z_full_grid(e, sw), false, "input planes short");
        e = d;
        e.z_out_lo = 1;
        expect(z_full_grid(e, sw), false, "first output plane cropped");
        e = d;
        e.z_out_hi = d.nz - 1;
        expect(z_full_grid(e, sw), false, "last output plane cropped");
        e = d;
        e.y_out_hi = d.ny - 16;   // (rows are the y and x passes' business)
        expect(z_full_grid(e, sw), true, "only rows cropped");
        NativeSwitches g;
        g.z_general = true;
        expect(z_full_grid(d, g), false, "MI_FFT_Z_GENERAL");
        NativeSwitches np_;
        np_.no_pair = true;
        NativeDims p{};
        plan_geometry(F, np_, &p, &sz);
        expect(p.paired == 0 && !z_full_grid(p, np_), true, "plain layout: no paired z pass, no form");
        checked += 7;
    }
    std::printf("checked %d failures %d\n", checked, failures);
    return failures;
}
