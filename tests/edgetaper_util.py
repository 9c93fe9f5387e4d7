"""Plain restatement of where csrc/edgetaper.hip and the direct engine's EPI_TAPER_SHELL epilogue do NOT compute, and the cases
of tests/test_gpu_edgetaper.py with the branch that each one is meant to reach.

  plateau   the samples of an axis whose taper value is exactly 1 (R.make_taper cuts ramp | ones | ramp to n, so the plateau is
            [w, n - w + 1) for n > 2 w and not symmetric); the blend leaves a voxel alone when it lies on the plateau of all
            three axes, and the blur is only needed elsewhere;
  tiles     the direct engine (csrc/conv3d_direct.hip) computes 128 x 16 x 2 outputs (x, y, z) per work-group and returns early,
            leaving `work` unwritten, for a tile that lies wholly on the plateau of all three axes.

Shapes are (z, y, x) throughout, like the arrays.  Tolerance of the GPU tests: the reference's own, max |got - want| < 1e-5 on
blocks drawn from [0, 1) (edgetaper_3d_test.m:4,40); nothing here widens it.
"""
import numpy as np

from oracle import rl_oracle as R
from tests.rl_util import asymmetric_psf

TILE = (2, 16, 128)   # TZ, TILE_Y, TILE_X of conv3d_direct.hip
BOUND = 1e-5          # edgetaper_3d_test.m:4,40
ENGINES = ("direct", "fft", "slabs")   # MI_EDGETAPER_ENGINE (the library reads the first letter)


def plateau(taper):
    """[lo, hi) of the samples that are exactly 1; they are contiguous for every taper make_taper builds."""
    ones = np.flatnonzero(np.asarray(taper) == np.float32(1.0))
    assert ones.size > 0, "make_taper always leaves a sample at 1"
    lo, hi = int(ones[0]), int(ones[-1]) + 1
    assert ones.size == hi - lo
    return lo, hi


def plateaus(shape, kshape):
    """Per axis (z, y, x): the plateau of the mask vectors edgetaper_3d uses for this block and PSF."""
    return [plateau(t) for t in R.edgetaper_mask_vectors(shape, kshape)]


def mask(shape, kshape):
    """The taper mask in float32, built x, then y, then z like the oracle and the kernel do."""
    tz, ty, tx = R.edgetaper_mask_vectors(shape, kshape)
    return (tx[None, None, :] * ty[None, :, None]).astype(np.float32) * tz[:, None, None]


def tile_grid(shape):
    """Every tile of the direct engine as ((z0, z1), (y0, y1), (x0, x1)), the last one of an axis cut to the block."""
    spans = [[(a, min(a + t, n)) for a in range(0, n, t)] for n, t in zip(shape, TILE)]
    return [(sz, sy, sx) for sz in spans[0] for sy in spans[1] for sx in spans[2]]


def skipped_tiles(shape, kshape):
    """The tiles wholly on the plateau of all three axes: the direct route must leave `work` untouched there."""
    plat = plateaus(shape, kshape)
    return [t for t in tile_grid(shape) if all(lo <= a and b <= hi for (a, b), (lo, hi) in zip(t, plat))]


def tile_centre(tile):
    return tuple((a + b) // 2 for a, b in tile)


def _gauss3(kshape):
    return R.gaussian_psf(kshape, [k / 5.0 for k in kshape]) * 3.0   # un-normalised on purpose (edgetaper_3d.m:14)


def _asym(kshape, scale=2.5):
    return asymmetric_psf(kshape, seed=sum(kshape)) * np.float32(scale)


# name -> shape (z, y, x), PSF extents (z, y, x), PSF builder, what the case is for
CASES = {
    # one 128 x 16 x 2 tile on the plateau: the early return of the direct route; rows longer than one stride of the blend
    "tile_skip_264": ((18, 40, 264), (7, 9, 9), _gauss3),
    # three skipped tiles along x; a plateau row of the blend jumps over two whole strides and lands in the third
    "three_strides_600": ((18, 40, 600), (5, 5, 7), _asym),
    # round(k / 2) = 12 > 8 along z: the ramp is 12 samples wide
    "wide_ramp": ((40, 20, 24), (23, 5, 5), _gauss3),
    # plateaus of one or two samples, and extents of 2 and 1 (n = 1: no taper on that axis at all)
    "degenerate_15_16_17": ((15, 16, 17), (3, 5, 7), _asym),
    "degenerate_17_15_16": ((17, 15, 16), (3, 5, 7), _asym),
    "degenerate_2_17_16": ((2, 17, 16), (3, 5, 7), _asym),
    "degenerate_1_20_33": ((1, 20, 33), (3, 5, 7), _asym),
    # every window reaches past both ends of the block
    "psf_larger_than_block": ((6, 7, 5), (9, 11, 13), _gauss3),
}
for _shape in ((18, 40, 264), (12, 20, 33)):
    for _k in ((4, 6, 8), (2, 2, 2), (6, 3, 4)):
        CASES["even_%dx%dx%d_k%d%d%d" % (_shape + _k)] = (_shape, _k, _asym)

ODD_CASES = sorted(n for n, c in CASES.items() if all(k % 2 for k in c[1]))
EVEN_CASES = sorted(n for n, c in CASES.items() if not all(k % 2 for k in c[1]))

_cache = {}


def case(name):
    """(bl, psf, want, mask) of a case, computed once: bl in [0, 1), want = R.edgetaper_3d(bl, psf) (float64 accumulation).
    The arrays are shared between the tests and must not be written to."""
    if name not in _cache:
        shape, kshape, make_psf = CASES[name]
        bl = np.random.default_rng(4000 + sorted(CASES).index(name)).random(shape, dtype=np.float32)
        psf = np.ascontiguousarray(make_psf(kshape), dtype=np.float32)
        assert psf.shape == tuple(kshape)
        out = (bl, psf, R.edgetaper_3d(bl, psf), mask(shape, kshape))
        for a in out:
            a.setflags(write=False)
        _cache[name] = out
    return _cache[name]


def report(line):
    print("[edgetaper] " + line, flush=True)
