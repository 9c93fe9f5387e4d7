"""Host check of the OTF factorisation (csrc/otf_factor.h), compiled with g++ and run without a device
(tests/host/otf_factor_check.cpp): which PSFs are adopted, at which rank, and what the tables built from the factors stand for.

The bound is the header's own: sum|psf - sum_r a_r (x) B_r| <= 2^-23 sum|psf| at the smallest R <= 4, which keeps every OTF entry
within 2^-23 of the OTF's largest entry (every entry is a sum of PSF samples times factors of modulus <= 1).

The symmetrised random PSF: a 7 x 7 x 7 array that is even in z has only four different z planes, so its (z) x (y x) unfolding has
rank 4 and four terms reproduce it exactly -- it is adopted, at exactly R = 4, and that is asserted.  The refusal of a symmetric PSF
of higher rank is shown on 11 x 7 x 7 (six different planes)."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import real_otf_util as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = 2.0 ** -23


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("otf_factor") / "otf_factor_check")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(ROOT, "image-preprocessing-pipeline_amd", "csrc"), "-o", out,
                    os.path.join(ROOT, "tests", "host", "otf_factor_check.cpp")], check=True)
    return out


def _factor(exe, psf, tmp_path, grid=None):
    """(rank, [resid after 1..4 terms], reconstructed OTF on ``grid`` or None)"""
    psf = np.ascontiguousarray(psf, np.float32)
    raw = str(tmp_path / "psf.raw")
    psf.tofile(raw)
    cmd = [exe, "otf" if grid else "factor", raw] + [str(k) for k in psf.shape]
    if grid:
        cmd += [str(f) for f in grid] + [str(tmp_path / "otf.raw")]
    run = subprocess.run(cmd, capture_output=True, text=True)
    assert run.returncode == 0, (run.returncode, run.stdout, run.stderr)
    m = re.search(r"rank (\d+) resid (\S+) (\S+) (\S+) (\S+)", run.stdout)
    assert m, run.stdout
    otf = np.fromfile(str(tmp_path / "otf.raw"), np.float64).reshape(grid) if grid else None
    return int(m.group(1)), [float(m.group(i)) for i in range(2, 6)], otf


def _psfs_of_real_use():
    import bench
    from ipp_amd import psf as P
    out = {name: bench.make_psf(bench.WORKLOADS[name][1]) for name in ("c2", "c3", "c4")}
    out["dxy422_dz1000_matlab"] = P.generate_psf(dxy=422.0, dz=1000.0, flavour="matlab")[0]
    out["defaults"] = P.generate_psf()[0]
    return out


def symmetrised_random(kshape, seed=77):
    p = np.random.default_rng(seed).random(kshape) + 0.05
    for ax in range(3):
        p = p + np.flip(p, ax)
    return np.ascontiguousarray((p / p.sum()).astype(np.float32))


def three_term_psf(kshape=(9, 7, 7), seed=5):
    """Three terms even(z) (x) B(y, x) with B point-symmetric but not separable and not mirror-symmetric per axis."""
    rng = np.random.default_rng(seed)
    kz, ky, kx = kshape
    z = np.arange(kz) - kz // 2
    yy, xx = np.meshgrid(np.arange(ky) - ky // 2, np.arange(kx) - kx // 2, indexing="ij")
    p = np.zeros(kshape)
    for r, (w, sz) in enumerate(((1.0, 1.2), (0.3, 2.5), (0.05, 0.7))):
        a = np.exp(-0.5 * (z / sz) ** 2)
        b = np.exp(-0.5 * ((yy / (1.0 + r)) ** 2 + (xx / (2.0 - 0.5 * r)) ** 2 + 0.6 * yy * xx / (1.0 + r)))   # sheared: B(y, x) != B(y, -x)
        b = b + 0.1 * rng.random() * np.cos(0.9 * (yy - xx))
        p += w * a[:, None, None] * b[None]
    assert np.all(p > 0)
    return np.ascontiguousarray((p / p.sum()).astype(np.float32))


def test_psfs_of_real_use_are_adopted_within_the_bound(exe, tmp_path):
    for name, psf in _psfs_of_real_use().items():
        assert all(k % 2 == 1 for k in psf.shape) and np.array_equal(psf, psf[::-1, ::-1, ::-1])
        rank, resid, _ = _factor(exe, psf, tmp_path)
        print(f"{name} {psf.shape}: rank {rank}, residual after 1..4 terms " + " ".join(f"{r:.2e}" for r in resid))
        assert 1 <= rank <= 4 and resid[rank - 1] <= BOUND
        assert all(r > BOUND for r in resid[:rank - 1])   # the smallest such R


def test_gaussian_is_rank_one(exe, tmp_path):
    from oracle import rl_oracle as R
    rank, resid, _ = _factor(exe, R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0)), tmp_path)
    print("gaussian:", rank, resid)
    assert rank == 1 and resid[0] <= BOUND


def test_symmetric_psfs_of_high_rank(exe, tmp_path):
    rank, resid, _ = _factor(exe, symmetrised_random((7, 7, 7)), tmp_path)
    print("7x7x7 symmetrised random:", rank, resid)
    assert rank == 4 and resid[2] > 1e-3 and resid[3] <= 1e-12   # four different z planes: exact at R = 4, far off at R = 3
    rank, resid, _ = _factor(exe, symmetrised_random((11, 7, 7)), tmp_path)
    print("11x7x7 symmetrised random:", rank, resid)
    assert rank == 0 and resid[3] > 1e-3


def test_asymmetric_psf_is_refused(exe, tmp_path):
    rank, resid, _ = _factor(exe, U.psf_family(1e-5), tmp_path)
    print("psf_family(1e-5):", rank, resid)
    assert rank == 0 and resid[3] > BOUND


@pytest.mark.parametrize("which", ["gaussian", "three_terms", "lightsheet"])
def test_tables_rebuild_the_otf(exe, tmp_path, which):
    from oracle import rl_oracle as R
    if which == "gaussian":
        psf = R.gaussian_psf((5, 7, 5), (1.0, 1.5, 1.0))
    elif which == "three_terms":
        psf = three_term_psf()
    else:
        import bench
        from ipp_amd import psf as P
        psf = P.resample_psf(bench.make_psf((31, 15, 15)), (15, 9, 9))
    grid = (64, 16, 32)
    rank, resid, got = _factor(exe, psf, tmp_path, grid)
    ratio, otf = U.imag_ratio(psf, grid)   # the float64 DFT of the PSF with its centre sample at the origin
    err = np.abs(got - otf.real).max() / np.abs(otf.real).max()
    print(f"{which}: rank {rank}, residual {resid[rank - 1]:.2e}, OTF error {err:.2e} of the largest entry (imaginary part {ratio:.1e})")
    assert 1 <= rank <= 4 and ratio < 1e-12
    assert err <= BOUND
