// db9 as destripe.hip (the z filter) and pystripe_wavelet.hip (the tile filter) share it: the table, the four float32 filters a
// kernel takes by value, and the half-point symmetric extension both transforms index through.
#pragma once
#include <hip/hip_runtime.h>

namespace mi {
namespace db9 {

constexpr int LF = 18;

// Lo_R = sqrt(2) * dbwavf('db9'): the extremal-phase Daubechies filter with 9 vanishing moments (published table; the tests
// recompute it by spectral factorisation of the half-band polynomial, agreement 3e-11)
constexpr double kLoR[LF] = {3.80779473638783381e-02,  2.43834674612590230e-01,  6.04823123690111153e-01,  6.57288078051299962e-01,
                             1.33197385825007591e-01,  -2.93273783279174305e-01, -9.68407832229760124e-02, 1.48540749338105876e-01,
                             3.07256814793338794e-02,  -6.76328290613307237e-02, 2.50947114831909018e-04,  2.23616621236789742e-02,
                             -4.72320475775138936e-03, -4.28150368246343286e-03, 1.84764688305622871e-03,  2.30385763523196190e-04,
                             -2.51963188942710503e-04, 3.93473203162716365e-05};

struct Filters {
    float lo_d[LF], hi_d[LF], lo_r[LF], hi_r[LF];
};

inline Filters make_filters() {
    Filters f;
    for (int t = 0; t < LF; ++t) {
        f.lo_r[t] = (float)kLoR[t];
        f.hi_r[t] = (float)(kLoR[LF - 1 - t] * ((t & 1) ? -1.0 : 1.0));   // qmf: reversed, the even (1-based) entries negated
    }
    for (int t = 0; t < LF; ++t) {
        f.lo_d[t] = f.lo_r[LF - 1 - t];
        f.hi_d[t] = f.hi_r[LF - 1 - t];
    }
    return f;
}

__device__ __forceinline__ int sym_index(int j, int n) {   // half-point symmetric extension, any distance
    const int p = 2 * n;
    j %= p;
    if (j < 0) j += p;
    return j < n ? j : p - 1 - j;
}

}  // namespace db9
}  // namespace mi
