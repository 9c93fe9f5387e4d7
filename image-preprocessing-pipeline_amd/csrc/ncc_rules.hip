// The host rules of MIP-NCC, bit-identical in float / int arithmetic to compute_funcs.cu:160-342,1294-1609 (argmax, peak widths,
// the alignment of an axis from two planes), the geometry of a pair and the one decision margin.  No device code.
#include <cstdlib>

#include "ncc_internal.h"

namespace mi {

// Resolution of the map values the fast paths produce (summed-area tables + blocked / lag-transform cross terms): a decision
// whose operands are closer than this is re-taken on entries recomputed in the two-pass form.  MI_NCC_MARGIN overrides (tests).
float ncc_margin() {
    static const float m = [] {
        const char* e = std::getenv("MI_NCC_MARGIN");
        return e ? (float)std::atof(e) : 4e-6f;
    }();
    return m;
}

// compute_MAX_ind (compute_funcs.cu:1294-1305)
int argmax_first(const float* v, int len) {
    float best = v[0];
    int ind = 0;
    for (int i = 0; i < len; ++i)
        if (v[i] > best) { best = v[i]; ind = i; }
    return ind;
}

// half width of the peak at `ind` along one direction of the (2*wR1+1) x (2*wR2+1) window
// (compute_NCC_width, compute_funcs.cu:160-282).  `second_bound` is the limit of the slope-projection
// loops, which the reference takes from the horizontal range for both directions (:252,267); where it
// exceeds this direction's own range the reference indexes outside the window, so it is clamped.
//
// `tight` (optional) receives the smallest margin, in NCC units, by which any comparison or rounding step below was decided: the
// caller re-decides on exactly recomputed entries when it is below the resolution of its map values (mi::ncc_margin()).
inline void note_margin(float* tight, float a, float b) {
    if (!tight) return;
    const float d = std::fabs(a - b);  // NaN operands: the comparison is false whatever their last bits are
    if (d < *tight) *tight = d;
}
// q is about to be floored; dq/dNCC ~ scale: the margin is the distance to the next integer in NCC units
inline void note_rounding(float* tight, float q, float scale) {
    if (!tight || !(q == q) || !(scale > 0.0f)) return;
    const float f = std::fmin(q - std::floor(q), std::ceil(q) - q);
    const float d = (q == std::floor(q) ? 0.0f : f) / scale;
    if (d < *tight) *tight = d;
}
int peak_half_width(const mi_ncc_params& P, const float* M, int ind, int step, int range, int second_bound, float* tight) {
#pragma clang fp contract(off)  // the float expression order below is part of the specification
    if (range < P.minDim_NCCmap) return P.INF_W;
    second_bound = imin(second_bound, range);
    const float thr = P.widthThr * M[ind];
    bool found = false;
    int w = 1;
    while (w <= range && !found) {
        note_margin(tight, M[ind - w * step], thr);
        if (M[ind - w * step] <= thr) found = true; else ++w;
    }
    found = false;
    while (w <= range && !found) {
        note_margin(tight, M[ind + w * step], thr);
        if (M[ind + w * step] <= thr) found = true; else ++w;
    }
    if (found) return w;
    float prec = M[ind - P.minPoints * step];
    int dist = P.minPoints + 1;
    while (dist <= second_bound && !found) {
        note_margin(tight, M[ind - dist * step], prec);
        if (M[ind - dist * step] >= prec) found = true;
        else { prec = M[ind - dist * step]; ++dist; }
    }
    if (dist < 2 * P.minPoints) w = P.INF_W;
    else {
        const float q = (float)((dist - 1) * (M[ind] - thr) / (M[ind] - prec));
        note_rounding(tight, q, (float)(dist - 1) / std::fabs(M[ind] - prec));
        w = (int)std::floor(q);
    }
    found = false;
    prec = M[ind + P.minPoints * step];
    dist = P.minPoints + 1;
    while (dist <= second_bound && !found) {
        note_margin(tight, M[ind + dist * step], prec);
        if (M[ind + dist * step] >= prec) found = true;
        else { prec = M[ind + dist * step]; ++dist; }
    }
    if (dist < 2 * P.minPoints) w = P.INF_W;
    else {
        const float q = (float)((dist - 1) * (M[ind] - thr) / (M[ind] - prec));
        note_rounding(tight, q, (float)(dist - 1) / std::fabs(M[ind] - prec));
        w = imin(imax(w, (int)std::floor(q)), P.INF_W - 1);
    }
    return w;
}

// compute_NCC_alignment (compute_funcs.cu:297-342)
void combine_axis(const mi_ncc_params& P, mi_ncc_descr* R, int ax, int d1, float p1, int w1, int d2, float p2, int w2, float* tight) {
#pragma clang fp contract(off)
    if (w1 == 1) w1 = P.INF_W;
    if (w2 == 1) w2 = P.INF_W;
    if (w1 < P.INF_W) note_margin(tight, p1, P.maxThr);
    if (w2 < P.INF_W) note_margin(tight, p2, P.maxThr);
    const bool ok1 = p1 >= P.maxThr && w1 < P.INF_W, ok2 = p2 >= P.maxThr && w2 < P.INF_W;
    int d;
    float p;
    int w;
    if (ok1 && ok2) {
        if (std::abs(d1 - d2) < imin(w1, w2)) {
            const float mean = (p1 * d1 + p2 * d2) / (p1 + p2);
            if (d1 != d2) note_rounding(tight, mean + 0.5f, (float)std::abs(d1 - d2) / (p1 + p2));
            d = (int)std::floor((double)mean + 0.5);
            p = (p1 * p1 + p2 * p2) / (p1 + p2);
            w = imax(w1, w2);
        } else {
            if (tight) { const float m = std::fabs(p1 / w1 - p2 / w2) * (float)imin(w1, w2); if (m < *tight) *tight = m; }
            if (p1 / w1 > p2 / w2) { d = d1; p = p1; w = w1; }
            else { d = d2; p = p2; w = w2; }
        }
    } else if (ok1) { d = d1; p = p1; w = w1; }
    else if (ok2) { d = d2; p = p2; w = w2; }
    else { d = P.INV_COORD; p = P.UNR_NCC; w = P.INF_W; }
    R->coord[ax] = d;
    R->NCC_maxs[ax] = p;
    R->NCC_widths[ax] = w;
}

int plan_pair(int dimk, int dimi, int dimj, int nk, int ni, int nj, int delayk, int delayi, int delayj, int side, mi_ncc_params* p,
              PairPlan& pl) {
    MI_REQUIRE(p, "CrossMIPs: missing configuration parameters");
    if (p->enhance) return fail(MI_ERR_UNSUPPORTED, "CrossMIPs: enhance is not built (PDAlgoMIPNCC.cpp:81 never enables it)");
    MI_REQUIRE(dimk > 0 && dimi > 0 && dimj > 0, "CrossMIPs: empty stack");
    MI_REQUIRE(nk == 0, "CrossMIPs: nk must be 0 (CrossMIPs.h: assumed 0 by the current implementation)");
    MI_REQUIRE(side == MI_NORTH_SOUTH || side == MI_WEST_EAST, "CrossMIPs: unexpected alignment configuration");
    MI_REQUIRE(ni >= 0 && nj >= 0 && ni < dimi && nj < dimj, "CrossMIPs: initial offsets outside the stack");
    MI_REQUIRE(delayi >= 0 && delayj >= 0 && delayk >= 0, "CrossMIPs: negative search range");
    MI_REQUIRE(!(p->wRangeThr_i > delayi || p->wRangeThr_j > delayj || p->wRangeThr_k > delayk),
               "CrossMIPs: one or more parameters: wRangeThr_i[=%d], wRangeThr_j[=%d], wRangeThr_k[=%d] are too large with respect to: "
               "delayi[=%d], delayj[=%d], delayik[=%d]",
               p->wRangeThr_i, p->wRangeThr_j, p->wRangeThr_k, delayi, delayj, delayk);
    MI_REQUIRE(p->wRangeThr_i >= 0 && p->wRangeThr_j >= 0 && p->wRangeThr_k >= 0 && p->minPoints >= 1 && p->maxIter >= 0,
               "CrossMIPs: invalid parameters");
    // libcrossmips.cpp:260-262,275-277
    delayi = imin(delayi, imax(0, dimi - ni - p->minDim_NCCsrc));
    delayj = imin(delayj, imax(0, dimj - nj - p->minDim_NCCsrc));
    delayk = imin(delayk, imax(0, dimk - nk - p->minDim_NCCsrc));
    p->wRangeThr_i = imin(p->wRangeThr_i, delayi);
    p->wRangeThr_j = imin(p->wRangeThr_j, delayj);
    p->wRangeThr_k = imin(p->wRangeThr_k, delayk);
    pl.dimk = dimk;
    pl.dimi_v = side == MI_NORTH_SOUTH ? dimi - ni : dimi;
    pl.dimj_v = side == MI_WEST_EAST ? dimj - nj : dimj;
    pl.ai0 = side == MI_NORTH_SOUTH ? ni : 0;
    pl.aj0 = side == MI_WEST_EAST ? nj : 0;
    pl.delayi = delayi; pl.delayj = delayj; pl.delayk = delayk;
    const int mu[3] = {pl.dimi_v, pl.dimi_v, pl.dimj_v}, mv[3] = {pl.dimj_v, dimk, dimk};
    const int du[3] = {delayi, delayi, delayj}, dv[3] = {delayj, delayk, delayk};
    const int wu[3] = {p->wRangeThr_i, p->wRangeThr_i, p->wRangeThr_j}, wv[3] = {p->wRangeThr_j, p->wRangeThr_k, p->wRangeThr_k};
    size_t off = 0;
    auto take = [&off](size_t n) { size_t o = off; off += (n + 3) / 4 * 4; return o; };
    for (int m = 0; m < 3; ++m) {
        PlaneGeom& g = pl.g[m];
        g.dimu = mu[m]; g.dimv = mv[m]; g.delayu = du[m]; g.delayv = dv[m]; g.wu = wu[m]; g.wv = wv[m];
        g.tiled = (g.dimu / TILE) * (g.dimv / TILE) > 0;
    }
    // MIPs first (one memset covers them), then tile sums, then maps (one D2H covers them)
    for (int m = 0; m < 3; ++m) pl.g[m].mip1 = take((size_t)pl.g[m].dimu * pl.g[m].dimv);
    for (int m = 0; m < 3; ++m) pl.g[m].mip2 = take((size_t)pl.g[m].dimu * pl.g[m].dimv);
    for (int m = 0; m < 3; ++m) {
        const size_t nt = (size_t)(pl.g[m].dimu / TILE) * (pl.g[m].dimv / TILE);
        pl.g[m].ps1 = take(nt);
        pl.g[m].ps2 = take(nt);
    }
    pl.map_begin = off;
    size_t res = 0;
    for (int m = 0; m < 3; ++m) {
        pl.g[m].map = take((size_t)(2 * du[m] + 1) * (2 * dv[m] + 1));
        res = std::max(res, (size_t)(2 * wu[m] + 1) * (2 * wv[m] + 1));
    }
    pl.map_floats = off - pl.map_begin;
    pl.res_floats = res;
    pl.total_floats = off;  // miss results live behind this
    size_t soff = 0;
    for (int m = 0; m < 3; ++m) {
        pl.g[m].sat = soff;
        soff += SatLayout(pl.g[m].dimu, pl.g[m].dimv).total;
    }
    pl.sat_doubles = soff;
    return MI_OK;
}

}  // namespace mi
