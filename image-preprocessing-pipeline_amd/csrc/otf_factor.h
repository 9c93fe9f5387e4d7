// The factored form of the real OTF as pure host functions (plain C++17, no device: tests/test_otf_factor_host.py compiles this header
// with g++).  A light-sheet PSF is, to float32 rounding, a sum of a few terms a_r(z) (x) B_r(y, x) -- excitation(z, x) times
// detection(x, y, z) at low NA -- so its centred OTF is Gr(kx, ky, kz) = sum_r A_r(kz) * Bh_r(kx, ky) with
//   A_r(kz)      = sum_z a_r(z) cos(2 pi kz (z - cz) / Fz)                                (a_r even about the centre sample)
//   Bh_r(kx, ky) = sum_{y,x} B_r(y, x) cos(2 pi (kx (x - cx) / Fx + ky (y - cy) / Fy))    (B_r point-symmetric about the centre)
// and the z pass can rebuild every entry from 4 Fz floats plus 8 floats per line pair instead of reading it (k_z_pair_pipe, FACT).
//
// otf_factor() finds the terms by rank-1 deflation of the (z) x (y * x) matrix with power iteration (never through the Gram matrix:
// sigma_4 / sigma_1 is about 1e-7, whose square is the edge of double precision).  Every term is replaced by its symmetric part --
// a_r by its even part, B_r by its point-symmetric part, which is what the cosine sums above see -- before it is subtracted, so the
// residual that decides is the residual of exactly what the tables stand for; a PSF that is not symmetric in this way keeps its
// antisymmetric part in the residual and is refused.  Adopted: the smallest R <= 4 with sum|psf - sum_r a_r (x) B_r| <= 2^-23 sum|psf|.
// Every OTF entry is a sum of PSF samples times factors of modulus <= 1, so that bound keeps every entry within one float32 ulp of the
// OTF's largest entry.
#pragma once
#include <cmath>
#include <cstddef>
#include <vector>

namespace mi {

constexpr int kOtfMaxRank = 4;
constexpr double kOtfFactorBound = 1.1920928955078125e-7;  // 2^-23

struct OtfFactors {
    int rank = 0;                  // 0: refused (the plan keeps the stored real form)
    int kx = 0, ky = 0, kz = 0;    // PSF extents
    double resid[kOtfMaxRank + 1] = {1, 1, 1, 1, 1};  // L1 residual after r terms, relative to sum|psf|
    std::vector<double> a;         // [r][kz]
    std::vector<double> b;         // [r][ky * kx]
};

// psf: [kz][ky][kx], extents odd (the centre sample is index k / 2 on every axis)
inline OtfFactors otf_factor(const float* psf, int kx, int ky, int kz) {
    OtfFactors f;
    f.kx = kx;
    f.ky = ky;
    f.kz = kz;
    if (kx <= 0 || ky <= 0 || kz <= 0 || !(kx & 1) || !(ky & 1) || !(kz & 1)) return f;
    const int m = kz, n = ky * kx;
    std::vector<double> e((size_t)m * n);
    double sum_abs = 0.0;
    for (size_t i = 0; i < e.size(); ++i) {
        e[i] = (double)psf[i];
        sum_abs += std::fabs(e[i]);
    }
    if (!(sum_abs > 0.0) || !std::isfinite(sum_abs)) return f;
    f.a.assign((size_t)kOtfMaxRank * m, 0.0);
    f.b.assign((size_t)kOtfMaxRank * n, 0.0);
    std::vector<double> u(m), v(n);
    for (int r = 0; r < kOtfMaxRank; ++r) {
        // start: the row of the residual with the largest norm
        int best = 0;
        double best_n = -1.0;
        for (int z = 0; z < m; ++z) {
            double q = 0.0;
            for (int j = 0; j < n; ++j) q += e[(size_t)z * n + j] * e[(size_t)z * n + j];
            if (q > best_n) { best_n = q; best = z; }
        }
        if (!(best_n > 0.0)) break;  // (squares underflowed: the residual stays above the bound, refused)
        for (int j = 0; j < n; ++j) v[j] = e[(size_t)best * n + j] / std::sqrt(best_n);
        double sigma = 0.0;
        for (int it = 0; it < 1000; ++it) {
            double un = 0.0;
            for (int z = 0; z < m; ++z) {
                double q = 0.0;
                for (int j = 0; j < n; ++j) q += e[(size_t)z * n + j] * v[j];
                u[z] = q;
                un += q * q;
            }
            un = std::sqrt(un);
            if (!(un > 0.0)) break;
            for (int z = 0; z < m; ++z) u[z] /= un;
            for (int j = 0; j < n; ++j) v[j] = 0.0;
            for (int z = 0; z < m; ++z)
                for (int j = 0; j < n; ++j) v[j] += u[z] * e[(size_t)z * n + j];
            double vn = 0.0;
            for (int j = 0; j < n; ++j) vn += v[j] * v[j];
            vn = std::sqrt(vn);
            if (!(vn > 0.0)) break;
            for (int j = 0; j < n; ++j) v[j] /= vn;
            const bool done = std::fabs(vn - sigma) <= 1e-15 * vn && it >= 2;
            sigma = vn;
            if (done) break;
        }
        // the symmetric part of the term: a even in z, B point-symmetric in (y, x)
        double* a = &f.a[(size_t)r * m];
        double* b = &f.b[(size_t)r * n];
        for (int z = 0; z < m; ++z) a[z] = 0.5 * sigma * (u[z] + u[m - 1 - z]);
        for (int j = 0; j < n; ++j) b[j] = 0.5 * (v[j] + v[n - 1 - j]);
        double res = 0.0;
        for (int z = 0; z < m; ++z)
            for (int j = 0; j < n; ++j) {
                e[(size_t)z * n + j] -= a[z] * b[j];
                res += std::fabs(e[(size_t)z * n + j]);
            }
        f.resid[r + 1] = res / sum_abs;
        for (int q = r + 2; q <= kOtfMaxRank; ++q) f.resid[q] = f.resid[r + 1];
        if (f.resid[r + 1] <= kOtfFactorBound) {
            f.rank = r + 1;
            break;
        }
    }
    for (int r = f.rank; r < kOtfMaxRank; ++r) {  // the unused ranks are zero: the tables have a single R
        for (int z = 0; z < m; ++z) f.a[(size_t)r * m + z] = 0.0;
        for (int j = 0; j < n; ++j) f.b[(size_t)r * n + j] = 0.0;
    }
    return f;
}

// cos / sin of 2 pi k d / F with the product reduced first
inline void otf_phase(long long k, long long d, long long F, double* c, double* s) {
    const long long t = ((k * d) % F + F) % F;
    const double two_pi = 6.283185307179586476925286766559;
    *c = std::cos(two_pi * (double)t / (double)F);
    *s = std::sin(two_pi * (double)t / (double)F);
}

// A_r(kz) on a grid of Fz planes
inline double otf_factor_A(const OtfFactors& f, int r, int kz, int Fz) {
    double acc = 0.0, c, s;
    for (int z = 0; z < f.kz; ++z) {
        otf_phase(kz, z - f.kz / 2, Fz, &c, &s);
        acc += f.a[(size_t)r * f.kz + z] * c;
    }
    return acc;
}

// the x half of Bh_r: C(y) = sum_x B_r(y, x) cos(theta_x), S(y) = sum_x B_r(y, x) sin(theta_x), theta_x = 2 pi kx (x - cx) / Fx
inline void otf_factor_B_x(const OtfFactors& f, int r, int kx, int Fx, double* C, double* S) {
    for (int y = 0; y < f.ky; ++y) {
        double cc = 0.0, ss = 0.0, c, s;
        for (int x = 0; x < f.kx; ++x) {
            otf_phase(kx, x - f.kx / 2, Fx, &c, &s);
            const double b = f.b[((size_t)r * f.ky + y) * f.kx + x];
            cc += b * c;
            ss += b * s;
        }
        C[y] = cc;
        S[y] = ss;
    }
}

// Bh_r(kx, ky) = sum_y cos(theta_y) C(y) - sin(theta_y) S(y)   (cos(theta_x + theta_y) split; the same sum the device table kernel takes)
inline double otf_factor_B(const OtfFactors& f, int r, int kx, int ky, int Fx, int Fy) {
    std::vector<double> C(f.ky), S(f.ky);
    otf_factor_B_x(f, r, kx, Fx, C.data(), S.data());
    double acc = 0.0, c, s;
    for (int y = 0; y < f.ky; ++y) {
        otf_phase(ky, y - f.ky / 2, Fy, &c, &s);
        acc += c * C[y] - s * S[y];
    }
    return acc;
}

}  // namespace mi
