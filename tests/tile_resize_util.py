"""Yardsticks of the tile resize (pystripe/core.py:1356-1359 without a pre-filter) and the input generator.

``zoom_ref`` is the yardstick: scipy's zoom and the clip, as DESIGN.md section 14 restates skimage's ``resize``.  ``recipe`` is the
arithmetic the kernels are built to, in numpy.  ``check_integer`` compares an integer result with ``zoom_ref`` where the float64
interpolant is safely away from an integer, and allows either neighbour where it is not (scipy's own last bit decides there)."""
import numpy as np

# every shape pair of the tests: growing, growing with rows of a multiple of 16 bytes, shrinking, one axis kept, mixed without a
# filter, several work-groups per row
CASES = (((37, 41), (53, 60)), ((9, 7), (20, 31)), ((1, 9), (4, 20)), ((64, 48), (80, 60)), ((45, 70), (19, 33)), ((128, 128), (107, 107)),
         ((300, 3), (125, 2)), ((33, 10), (33, 25)), ((34, 50), (34, 37)), ((40, 50), (30, 64)), ((6, 2100), (5, 2600)))
DTYPES = (np.uint8, np.uint16, np.float32)
SEEDS = (0, 1, 2)   # the tiles of one batch
# 4 products and 3 sums of at most half an ulp of 2^16 each (2^-37) stay below 2^-33; doubled for the two sides compared; times four
STRICT = 2.0 ** -30


def zoom_ref(tile, N):
    """``resize(tile, N, preserve_range=True, anti_aliasing=False)``: an integer tile as float64, a float32 tile as it is."""
    from scipy import ndimage
    a = tile if tile.dtype == np.float32 else tile.astype(np.float64)
    v = ndimage.zoom(a, [N[0] / tile.shape[0], N[1] / tile.shape[1]], order=1, mode="mirror", grid_mode=True)
    assert v.shape == tuple(N) and v.dtype == a.dtype
    return np.clip(v, a.min(), a.max())


def tables(n, m):
    """(i0, i1, t) of one axis, n samples -> m samples, in float64."""
    z = np.float64(n) / np.float64(m)
    c = (np.arange(m, dtype=np.float64) + 0.5) * z - 0.5
    if n == 1:
        c = np.zeros(m)
    else:
        c = np.where(c < 0, -c, c)
        c = np.where(c > n - 1, 2.0 * (n - 1) - c, c)
    fl = np.floor(c)
    i0 = fl.astype(np.int64)
    i1 = i0 + 1
    i1 = np.where(i1 > n - 1, 2 * (n - 1) - i1 if n > 1 else 0, i1)
    return i0.astype(np.int32), i1.astype(np.int32), c - fl


def recipe(tile, N):
    """Recipe R: the sum of the four products in float64, left to right; clipped; float32 rounded before the clip, integers
    truncated after it."""
    a = tile.astype(np.float64)
    y0, y1, ty = tables(tile.shape[0], N[0])
    x0, x1, tx = tables(tile.shape[1], N[1])
    s = None
    for yi, wy in ((y0, 1.0 - ty), (y1, ty)):
        for xi, wx in ((x0, 1.0 - tx), (x1, tx)):
            term = (a[yi][:, xi] * wy[:, None]) * wx[None, :]
            s = term if s is None else s + term
    if tile.dtype == np.float32:
        return np.clip(s.astype(np.float32), tile.min(), tile.max())
    return np.trunc(np.clip(s, a.min(), a.max())).astype(tile.dtype)


def pattern(shape, dtype, seed):
    """Random full-range samples, the top third of the rows at the type's maximum, a zero block in the lower-left quarter (an eighth
    of each extent, in the corner), one constant row (tiles of four rows or more); float32: the uint16 pattern / 7.3 - 100.  The flat
    parts interpolate to integers, so they are where truncation is decided by the last bit; they are kept small enough that, with
    SEEDS, more than half of the samples of every pair of CASES stay strict -- also of (33, 10) -> (33, 25), whose kept axis and
    weights of k / 10 leave only about 0.82 of the random part strict (tests/test_tile_resize_host.py checks every share)."""
    dtype = np.dtype(dtype)
    ny, nx = shape
    top = 255 if dtype == np.uint8 else 65535
    a = np.random.default_rng(seed).integers(0, top + 1, shape).astype(np.uint8 if dtype == np.uint8 else np.uint16)
    a[:ny // 3] = top
    a[ny - ny // 8:, :nx // 8] = 0
    if ny >= 4:
        a[ny // 2] = top // 3
    if dtype == np.float32:
        return (a.astype(np.float32) / np.float32(7.3) - np.float32(100)).astype(np.float32)
    return a


def strict_share(tile, N):
    v = zoom_ref(tile, N)
    return float((np.abs(v - np.rint(v)) > STRICT).mean())


def check_integer(got, tile, N, what="", convert=None, place=None):
    """``got`` against ``zoom_ref``: a strict sample (the interpolant further than 2^-30 from an integer) must be trunc(v); every
    other one rint(v) or rint(v) - 1, inside the tile's [min, max].  At least half of the samples must be strict.  When ``got`` went
    through more of process_img, ``convert`` is what follows value by value (the 8 / 16-bit conversion, on an array of the tile's
    type) and ``place`` what moves samples (flip, rotation); both are applied to the expected values before comparing."""
    convert = convert or (lambda a: a)
    place = place or (lambda a: a)
    v = zoom_ref(tile, N)
    near = np.rint(v)
    strict = np.abs(v - near) > STRICT
    share = float(strict.mean())
    assert share >= 0.5, f"{what}: only {share:.3f} of the samples are strict"
    lo, hi = float(tile.min()), float(tile.max())

    def expected(x):   # whole numbers as float64 -> (what process_img makes of them, whether they lie inside [min, max])
        return place(convert(np.clip(x, lo, hi).astype(tile.dtype))), place((x >= lo) & (x <= hi))

    want, _ = expected(np.trunc(v))
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    strict = place(strict)
    bad = strict & (got != want)
    assert not bad.any(), f"{what}: {int(bad.sum())} strict samples differ, first at {tuple(np.argwhere(bad)[0])}"
    (up, up_ok), (down, down_ok) = expected(near), expected(near - 1)
    bad = ~strict & ~(((got == up) & up_ok) | ((got == down) & down_ok))
    assert not bad.any(), f"{what}: {int(bad.sum())} near-integer samples are off, first at {tuple(np.argwhere(bad)[0])}"
    return share
