"""The foreground mask of filter_streaks (get_img_mask, pystripe/core.py:475-489) restated in numpy, step by step as
include/mi_tile_mask.h words it.  The morphology is written out as loops over the window's offsets; ``*_scipy`` is the same window
through scipy.ndimage's 1-D filters (tests/test_tile_mask_host.py holds the two against each other).  The fill labels the inverted
mask with scipy.ndimage.label and removes the labels of the four corners."""
import numpy as np
from scipy import ndimage

# the morphology cases of tests/test_gpu_tile_mask.py; tests/test_tile_mask_host.py checks that their expectations carry content
SHAPES = [(70, 130), (129, 257), (1, 300), (300, 1), (257, 65)]
BOXES = [(1, 1), (2, 1), (1, 2), (3, 4), (50, 7), (64, 65), (500, 500)]
# A box beyond ONE extent and inside the other: every box above 1 on the line tiles.  Beyond both: extreme_stack.

CROSS = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
FULL = np.ones((3, 3), bool)


def window(k):
    """offsets of the box along one axis: [-a, k - 1 - a] with OpenCV's default anchor a = k // 2"""
    a = k // 2
    return range(-a, k - a)


def _shifted(m, d, axis):
    """(destination slice, source slice) of ``out[i] op= m[i + d]`` for the i with 0 <= i + d < n"""
    n = m.shape[axis]
    lo, hi = max(0, -d), min(n, n - d)
    dst, src = [slice(None)] * m.ndim, [slice(None)] * m.ndim
    dst[axis], src[axis] = slice(lo, hi), slice(lo + d, hi + d)
    return tuple(dst), tuple(src)


def dilate1d(m, k, axis):
    """1 where any sample of the window that lies inside the tile is 1 (samples outside count as 0)"""
    out = np.zeros_like(m, dtype=bool)
    n = m.shape[axis]
    for d in window(k):
        if -n < d < n:
            dst, src = _shifted(m, d, axis)
            out[dst] |= m[src]
    return out


def erode1d(m, k, axis):
    """1 where every sample of the window that lies inside the tile is 1 (samples outside count as 1)"""
    out = np.ones_like(m, dtype=bool)
    n = m.shape[axis]
    for d in window(k):
        if -n < d < n:
            dst, src = _shifted(m, d, axis)
            out[dst] &= m[src]
    return out


def dilate(m, k):
    return dilate1d(dilate1d(m, k, 1), k, 0)


def erode(m, k):
    return erode1d(erode1d(m, k, 1), k, 0)


def close_open(m, close_steps, open_steps):
    m = erode(dilate(m, close_steps), close_steps)
    return dilate(erode(m, open_steps), open_steps)


def _scipy1d(m, k, axis, dilation):
    """the same window through scipy: origin=0 places a filter of size k over [i - k // 2, i - k // 2 + k - 1]"""
    n = m.shape[axis]
    if k > 2 * n:     # the window covers the line from every sample: scipy would only pad for longer
        k = 2 * n + (k % 2)
    u = m.astype(np.uint8)
    if dilation:
        return ndimage.maximum_filter1d(u, k, axis=axis, mode="constant", cval=0, origin=0).astype(bool)
    return ndimage.minimum_filter1d(u, k, axis=axis, mode="constant", cval=1, origin=0).astype(bool)


def close_open_scipy(m, close_steps, open_steps):
    for k, order in ((close_steps, (True, False)), (open_steps, (False, True))):
        for dilation in order:
            m = _scipy1d(_scipy1d(m, k, 1, dilation), k, 0, dilation)
    return m


def fill(m, connectivity=4):
    """m | (the regions of ~m that hold none of the four corner samples)"""
    inv = ~m
    labels, _ = ndimage.label(inv, structure=CROSS if connectivity == 4 else FULL)
    corners = {int(labels[y, x]) for y in (0, -1) for x in (0, -1)} - {0}
    removed = np.isin(labels, sorted(corners)) if corners else np.zeros_like(m)
    return m | (inv & ~removed)


def threshold(img, thr, log_domain=False):
    """img > thr; float tiles compare in float32 (NaN gives 0), ``log_domain`` compares numpy's float32 log1p"""
    img = np.asarray(img)
    if img.dtype.kind == "f":
        with np.errstate(invalid="ignore"):
            v = np.log1p(img, dtype=np.float32) if log_domain else img
            return v > np.float32(thr)
    return img > thr


def get_img_mask(img, thr, close_steps=50, open_steps=500, connectivity=4, log_domain=False):
    """the mask of one 2-D tile, bool"""
    return fill(close_open(threshold(img, thr, log_domain), close_steps, open_steps), connectivity)


def framed(m):
    """``m`` with its border samples set: no background region then holds a corner, and none touches the border"""
    m = m.copy()
    m[0, :] = m[-1, :] = True
    m[:, 0] = m[:, -1] = True
    return m


def blobs(shape, seed, density=0.5, smooth=2):
    """a random binary image with structure at several scales: white noise, box-averaged ``smooth`` times, cut at its quantile"""
    rng = np.random.default_rng(seed)
    f = rng.random(shape)
    for _ in range(smooth):
        f = ndimage.uniform_filter(f, size=(min(5, shape[0]), min(5, shape[1])), mode="nearest")
    return f > np.quantile(f, 1 - density)


def serpentine(ny=65, nx=67):
    """foreground everywhere but a one-sample corridor that starts at the top-left corner and winds down the tile: the even rows,
    joined at alternating ends.  The corridor is the only background, so with the fill it is removed entirely."""
    m = np.ones((ny, nx), bool)
    for j, y in enumerate(range(0, ny, 2)):
        m[y, :] = False
        if y + 1 < ny:
            m[y + 1, nx - 1 if j % 2 == 0 else 0] = False
    return m


def structures(shape, kmax, seed=0):
    """Solid foreground structures on one background region that holds corners, so the fill removes exactly the background and the
    mask is the morphology's own result.  Whatever the boxes: a band along the first samples of the tile (it touches three borders),
    blocks a gap of 25 apart (a box of 50 closes it, a box below 26 does not) and far from the band, a structure across the word
    and wave edge at 63 / 64 and one across the work-group edge at 255 / 256 where the tile reaches them, one on the last samples.
    For boxes below 10 (``kmax``) also fine structure: sparse dots, bars with gaps of 1, 2 and 3 samples, single samples on the
    borders; on a tile narrower than 200 the structure at 63 / 64 is left out for larger boxes, which would join it to everything.
    A line tile (an extent of 1) gets segments away from its ends."""
    ny, nx = shape
    rng = np.random.default_rng(seed + 7 * ny + nx)
    m = np.zeros(shape, bool)
    if min(shape) == 1:   # on a line the fill closes every gap between two segments: the mask is the span the morphology leaves
        line = np.zeros(max(shape), bool)
        line[60:140] = True             # across 63 / 64; 60 from the line's start, which no box below 120 reaches
        line[250:262] = True            # across 255 / 256; 38 from the line's end
        if kmax < 10:
            line[12] = True             # an opening of 2 or more removes it, so the span starts later
            line[20:24] = line[30:36] = line[270:273] = line[285:287] = True
        return line.reshape(shape).copy()
    band = max(3, min(nx // 3, 45))
    m[:, :band] = True
    x0 = nx - 30 if nx < 100 else nx - 50 if nx <= 256 else 120
    m[5:20, x0:x0 + 15] = True
    m[45:60, x0:x0 + 15] = True         # 25 rows below the first block
    if nx > 80 and (kmax < 10 or nx > 200):
        m[ny // 2 - 4:ny // 2 + 6, 58:70] = True          # across 63 / 64
    if nx > 256:
        m[ny - 30:ny - 12, 246:266] = True                # across 255 / 256
    if ny > 256:
        m[250:262, band + 4:band + 14] = True             # across row 255 / 256
        m[ny - 4:, nx - 25:nx - 5] = True                 # on the last rows
    if kmax < 10:
        free = np.zeros(shape, bool)
        free[22:43, band + 6:] = True                     # between the blocks' rows, right of the band
        m |= free & (rng.random(shape) < 0.12)
        y = min(ny - 6, 64)
        for gap, xs in ((1, band + 8), (2, band + 20), (3, band + 32)):
            if xs + 2 * 6 + gap < nx:
                m[y:y + 5, xs:xs + 6] = True
                m[y:y + 5, xs + 6 + gap:xs + 12 + gap] = True
        m[0, nx // 2] = m[ny - 1, nx // 2 + 3] = m[ny // 2, nx - 1] = True
    return m


def extreme_stack(shape):
    """[empty, one sample, full but one sample, full]: what a box beyond both extents tells apart (a dilation is "any", an erosion "all")"""
    ny, nx = shape
    t = np.zeros((4,) + tuple(shape), bool)
    t[1, ny // 2, nx // 3] = True
    t[2] = True
    t[2, ny // 2, nx // 2] = False      # the centre lies in every sample's window once k / 2 - 1 reaches half the extent
    t[3] = True
    return t
