// Host check of csrc/fft_native_route.h (tests/test_fft_native_route_host.py): the length table against its case lists, and
// plan_geometry / z_route / y_route / x_route against the literal tables of fft_route_tables.h.  Prints one line per failure and
// a summary "checked <rows> failures <n>".
#include <cstdio>
#include <cstring>
#include <set>

#include "fft_native_route.h"

using namespace mi;

struct GeoRow {
    int F[3], sw, status;
    int dims[sizeof(NativeDims) / sizeof(int)];
    unsigned long long n_cplx, n_buf, gap;
    size_t tw_at[3], tw_total;
};
struct RouteRow {
    int F[3], sw, x_pipe_ok, z_pipe_ok, real_otf_possible, y_paired, z_plain, z_real, ph;
};
#include "fft_route_tables.h"

static int failures = 0, rows = 0;
#define CHECK(cond, ...) do { ++rows; if (!(cond)) { ++failures; std::printf("FAIL " __VA_ARGS__); std::printf("\n"); } } while (0)

static NativeSwitches switch_set(int k) {
    NativeSwitches w;
    if (k == 1) w.no_pair = true;
    if (k == 2) w.no_pipe = true;
    if (k == 3) w.no_xpipe = true;
    if (k == 4) w.complex_otf = true;
    if (k == 5) w.dbg = 8;
    if (k == 6) w.tl = 4;
    if (k == 7) { w.ty = 8; w.tc = 8; w.zpad = 3; w.xpad = 5; w.stgap = 1000 & ~127; }
    return w;
}

static void lengths() {
    const int* lists[3] = {kLengths0, kLengths1, kLengths2};
    int cases[3] = {0, 0, 0}, zq = 0;
    // every case is reachable: its length splits back into itself on the axes that take it
#define CASE(LG, R) for (int a = 0; a < 3; ++a) { int r = 0, l = 0; const bool z_long = a == 2 && (R << LG) > kMaxZ; \
        CHECK(split_axis(R << LG, a, &r, &l) == !z_long && (z_long || (r == R && l == LG)), "case (%d, %d) on axis %d", LG, R, a); cases[a] += !z_long; }
    MI_AXIS_CASES(CASE)
#undef CASE
#define CASE(LG, R) { int r = 0, l = 0; CHECK(split_axis(R << LG, 1, &r, &l) && r == R && l == LG && !split_axis(R << LG, 0, &r, &l) && \
        !split_axis(R << LG, 2, &r, &l), "y-only case (%d, %d)", LG, R); ++cases[1]; }
    MI_Y_ONLY_CASES(CASE)
#undef CASE
    // the paired list is a subset of the z list
#define CASE(LG, R, NTH, PH) { int nth = 0; bool ph = !PH; CHECK(axis_takes(2, LG, R) && z_pair_takes(LG, R, &nth, &ph) && nth == NTH && ph == PH, \
        "paired case (%d, %d)", LG, R); ++zq; }
    MI_ZQ_CASES(CASE)
#undef CASE
    int paired = 0;
    for (int l = 0; l < 16; ++l)
        for (int r = 1; r <= 9; ++r) paired += z_pair_takes(l, r);
    CHECK(paired == zq, "paired lengths %d, cases %d", paired, zq);
    for (int a = 0; a < 3; ++a) {
        std::set<int> want;
        for (const int* p = lists[a]; *p; ++p) want.insert(*p);
        int taken = 0;
        for (int n = 1; n <= 4608; ++n) {
            int r = 0, l = 0;
            const bool t = split_axis(n, a, &r, &l);
            taken += t;
            CHECK(t == (want.count(n) != 0) && (!t || (r << l) == n), "axis %d length %d: taken %d", a, n, (int)t);
        }
        CHECK(taken == cases[a], "axis %d: %d lengths accepted, %d cases", a, taken, cases[a]);  // every accepted length has a case
        CHECK(axis_longest(a) == *want.rbegin(), "axis %d: longest %d", a, axis_longest(a));
        for (int n = 1; n <= 9300; ++n) {  // good_size: the smallest accepted extent >= n
            const auto it = want.lower_bound(a == 0 ? (n + 1) / 2 : n);
            const int g = it == want.end() ? 0 : (a == 0 ? 2 * *it : *it);
            CHECK(native_good_size(n, a) == g, "good_size(%d, %d) = %d, want %d", n, a, native_good_size(n, a), g);
        }
    }
    for (const auto& g : kGoodSize) CHECK(native_good_size(g[1], g[0]) == g[2], "good_size(%d, %d) = %d, want %d", g[1], g[0], native_good_size(g[1], g[0]), g[2]);
    for (int x = 2; x <= 9216; x += 2) {  // supported() is the three splits together (a few y and z against every x)
        const int ys[] = {8, 24, 40, 100, 160, 4608}, zs[] = {8, 100, 2304, 4096};
        for (int y : ys)
            for (int z : zs) {
                const int F[3] = {x, y, z};
                int r, l;
                CHECK(native_supported(F) == (split_axis(x / 2, 0, &r, &l) && split_axis(y, 1, &r, &l) && split_axis(z, 2, &r, &l)), "supported(%d, %d, %d)", x, y, z);
            }
    }
    const int odd[3] = {129, 64, 64};
    CHECK(!native_supported(odd), "odd x");
}

static void geometry() {
    for (const GeoRow& g : kGeo) {
        NativeDims d;
        NativeSizes sz;
        std::memset(&d, 0, sizeof d);
        std::memset(&sz, 0, sizeof sz);
        const NativeSwitches w = switch_set(g.sw);
        const int rc = plan_geometry(g.F, w, &d, &sz);
        CHECK(rc == g.status, "geometry (%d, %d, %d) switches %d: status %d, want %d", g.F[0], g.F[1], g.F[2], g.sw, rc, g.status);
        if (rc != 0 || g.status != 0) continue;
        CHECK(std::memcmp(&d, g.dims, sizeof d) == 0, "geometry (%d, %d, %d) switches %d: dims differ (paired %d zpad %d xrow %d ty %d tc %d tl %d)", g.F[0],
              g.F[1], g.F[2], g.sw, d.paired, d.zpad, d.xrow, d.ty, d.tc, d.tl);
        CHECK(sz.n_cplx == g.n_cplx && sz.n_buf == g.n_buf && w.stgap == g.gap && sz.tw_at[0] == g.tw_at[0] && sz.tw_at[1] == g.tw_at[1] &&
                  sz.tw_at[2] == g.tw_at[2] && sz.tw_total == g.tw_total,
              "geometry (%d, %d, %d) switches %d: sizes differ (n_buf %zu)", g.F[0], g.F[1], g.F[2], g.sw, sz.n_buf);
    }
}

static void routes() {
    for (const RouteRow& r : kRoutes) {
        NativeDims d;
        NativeSizes sz;
        const NativeSwitches w = switch_set(r.sw);
        if (plan_geometry(r.F, w, &d, &sz) != 0) { CHECK(false, "routes (%d, %d, %d) switches %d: no geometry", r.F[0], r.F[1], r.F[2], r.sw); continue; }
        bool ph = true;
        if (d.paired) z_pair_takes(d.lz2, d.r3z, nullptr, &ph);
        CHECK(x_pipe_ok(d, w) == (r.x_pipe_ok != 0) && z_pipe_ok(d, w) == (r.z_pipe_ok != 0) && real_otf_possible(d, w) == (r.real_otf_possible != 0) &&
                  (y_route(d) == YRoute::pair) == (r.y_paired != 0) && (int)z_route(d, w, false) == r.z_plain && (int)z_route(d, w, true) == r.z_real &&
                  (!d.paired || ph == (r.ph != 0)),
              "routes (%d, %d, %d) switches %d: x_pipe_ok %d z_pipe_ok %d real possible %d y pair %d z %d / %d ph %d", r.F[0], r.F[1], r.F[2], r.sw,
              (int)x_pipe_ok(d, w), (int)z_pipe_ok(d, w), (int)real_otf_possible(d, w), (int)(y_route(d) == YRoute::pair), (int)z_route(d, w, false),
              (int)z_route(d, w, true), (int)ph);
    }
    // x: the plan facts (pipe_ok through MI_FFT_NO_PIPE on one grid, five pad windows, MI_FFT_NO_XPIPE) times the call facts
    PadWindow pws[5];
    pws[1].on = 1; pws[1].n[0] = 40; pws[1].n[1] = 30; pws[1].n[2] = 20;
    pws[2] = pws[1]; pws[2].n[0] = 42;
    pws[3] = pws[1]; pws[3].o[1] = 2;
    pws[4] = pws[1]; pws[4].rep[2] = 1;
    const char name[] = {'f', 'u', 'i', 'F', 'I', 'U', 'E'};  // in the order of XRoute
    const int F[3] = {128, 64, 64};
    const char* want = kXRoutes;
    size_t left = sizeof(kXRoutes) - 1;
    for (int pok = 0; pok < 2; ++pok)
        for (int wdw = 0; wdw < 5; ++wdw)
            for (int nox = 0; nox < 2; ++nox) {
                NativeSwitches w;
                w.no_pipe = !pok;
                w.no_xpipe = nox != 0;
                NativeDims d;
                NativeSizes sz;
                CHECK(plan_geometry(F, w, &d, &sz) == 0 && x_pipe_ok(d, w) == (pok != 0), "x routes: plan");
                const PadWindow& pw = pws[wdw];
                for (int al = 0; al < 2; ++al) {
                    XCall c;
                    c.forward = true;
                    c.aligned = al != 0;
                    const char got = name[(int)x_route(d, w, pw, c)];
                    CHECK(left && got == *want, "x_forward pipe_ok %d window %d no_xpipe %d aligned %d: %c, want %c", pok, wdw, nox, al, got, left ? *want : '?');
                    if (left) { ++want; --left; }
                }
                for (int epi = 0; epi < 5; ++epi)
                    for (int fuse = 0; fuse < 2; ++fuse)
                        for (int whole = 0; whole < 2; ++whole)
                            for (int al = 0; al < 2; ++al)
                                for (int out = 0; out < 2; ++out) {
                                    XCall c;
                                    c.fuse_forward = fuse != 0;
                                    c.whole = whole != 0;
                                    c.aligned = al != 0;
                                    c.ek = epi == 4 ? 0 : epi;
                                    c.taper_shell = epi == 4;
                                    c.has_out = out != 0;
                                    // x_inverse refuses these before it asks for a route
                                    const bool refused = fuse && (!(c.ek == 1 || c.ek == 2) || !pad_can_fuse(pw));
                                    const char got = refused ? 'x' : name[(int)x_route(d, w, pw, c)];
                                    CHECK(left && got == *want, "x_inverse pipe_ok %d window %d no_xpipe %d epi %d fuse %d whole %d aligned %d out %d: %c, want %c",
                                          pok, wdw, nox, epi, fuse, whole, al, out, got, left ? *want : '?');
                                    if (left) { ++want; --left; }
                                }
            }
    CHECK(left == 0, "x routes: %zu table entries left", left);
}

int main() {
    lengths();
    const int after_lengths = rows;
    geometry();
    routes();
    std::printf("checked %d (lengths %d, geometry and routes %d) failures %d\n", rows, after_lengths, rows - after_lengths, failures);
    return failures ? 1 : 0;
}
