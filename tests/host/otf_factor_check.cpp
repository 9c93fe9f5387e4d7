// Host driver of csrc/otf_factor.h for tests/test_otf_factor_host.py (no device).
//   otf_factor_check factor <psf.raw> kz ky kx
//       prints "rank R resid r1 r2 r3 r4" for the float32 PSF [kz][ky][kx] of the raw file
//   otf_factor_check otf <psf.raw> kz ky kx Fz Fy Fx <out.raw>
//       also writes sum_r A_r(kz) * Bh_r(kx, ky) for every frequency of the Fz x Fy x Fx grid as float64 [Fz][Fy][Fx]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "otf_factor.h"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    const bool want_otf = std::strcmp(argv[1], "otf") == 0;
    if (want_otf && argc < 10) return 2;
    const int kz = std::atoi(argv[3]), ky = std::atoi(argv[4]), kx = std::atoi(argv[5]);
    std::vector<float> psf((size_t)kz * ky * kx);
    FILE* fp = std::fopen(argv[2], "rb");
    if (!fp || std::fread(psf.data(), sizeof(float), psf.size(), fp) != psf.size()) return 3;
    std::fclose(fp);
    const mi::OtfFactors f = mi::otf_factor(psf.data(), kx, ky, kz);
    std::printf("rank %d resid %.6e %.6e %.6e %.6e\n", f.rank, f.resid[1], f.resid[2], f.resid[3], f.resid[4]);
    if (!want_otf) return 0;
    if (f.rank == 0) return 4;
    const int Fz = std::atoi(argv[6]), Fy = std::atoi(argv[7]), Fx = std::atoi(argv[8]);
    std::vector<double> A((size_t)mi::kOtfMaxRank * Fz), B((size_t)mi::kOtfMaxRank * Fy * Fx), out((size_t)Fz * Fy * Fx);
    for (int r = 0; r < mi::kOtfMaxRank; ++r) {
        for (int z = 0; z < Fz; ++z) A[(size_t)r * Fz + z] = mi::otf_factor_A(f, r, z, Fz);
        for (int y = 0; y < Fy; ++y)
            for (int x = 0; x < Fx; ++x) B[((size_t)r * Fy + y) * Fx + x] = mi::otf_factor_B(f, r, x, y, Fx, Fy);
    }
    for (int z = 0; z < Fz; ++z)
        for (int y = 0; y < Fy; ++y)
            for (int x = 0; x < Fx; ++x) {
                double g = 0.0;
                for (int r = 0; r < mi::kOtfMaxRank; ++r) g += A[(size_t)r * Fz + z] * B[((size_t)r * Fy + y) * Fx + x];
                out[((size_t)z * Fy + y) * Fx + x] = g;
            }
    FILE* fo = std::fopen(argv[9], "wb");
    if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) return 5;
    std::fclose(fo);
    return 0;
}
