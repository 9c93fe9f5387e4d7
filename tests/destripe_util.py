"""TEST INFRASTRUCTURE for mi_destripe_z (csrc/destripe.hip): a float64 reference composed of the building blocks of
oracle/destripe_oracle.py, the test volumes, guarded device buffers and the table of shapes that tests/test_gpu_destripe.py and
tests/test_destripe_util_host.py share.  Host only except ``guarded`` / ``assert_guards_intact``, which import torch when called.

The oracle's ``filter_subband_3d_z`` computes in float32, so a comparison with it is one float32 sum against another.  Its
blocks (``dwt_axis``, ``idwt_axis``, ``wavedec2``, ``waverec2``) take their precision from the array they are given;
``filter_subband_3d_z_f64`` hands them float64 data and restates only the glue around them."""
import functools
import os

import numpy as np

from oracle import destripe_oracle as D

SENTINEL = -12345.0

# constants of csrc/destripe.hip, restated (the host test derives from them which paths a shape reaches)
LF = 18
K_TILE_A = 512        # kTileA: outputs of k_dwt_x per work-group
K_TILE_X = 256        # kTileX: pairs of k_idwt_x per work-group
SEGMENT = 2 * K_TILE_A + 20   # the 1044 samples k_dwt_x stages per work-group, seg[q] = x[2 i0 - 16 + q]


def report(line):
    """Prints a measured figure; DESTRIPE_REPORT=<file> appends it to a file as well."""
    print(line)
    path = os.environ.get("DESTRIPE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


# ------------------------------------------------------------------------------------------------------- float64 reference
def _notch_f64(H, sigma):
    """filter_subband_3d_z.m:92-123 along z (axis 1 of a [X, Z] sub-band): real(ifft(fft(H, z) * (g + 1j g))) in float64.  g is
    built in single precision exactly as the reference builds it -- that is its rule, not rounding noise."""
    n = H.shape[1]
    g = D.gaussian_notch_filter_1d(n, max(float(sigma) / n, float(D.EPS_SINGLE))).astype(np.float64)[None, :]
    return np.real(np.fft.ifft(np.fft.fft(H, axis=1) * (g + 1j * g), axis=1))


def _slice_f64(img, sigma, levels, filters):
    pad = [s % 2 for s in img.shape]
    img = np.pad(img, [(0, pad[0]), (0, pad[1])])
    levels = levels or D.wmaxlev(img.shape, len(filters[0]))
    a, details, sizes = D.wavedec2(img, levels, filters)
    assert a.dtype == np.float64
    details = [(_notch_f64(H, sigma), V, Dd) for H, V, Dd in details]
    img = D.waverec2(a, details, sizes, filters)
    return img[:img.shape[0] - pad[0], :img.shape[1] - pad[1]]


def filter_subband_3d_z_f64(bl, sigma, levels=0):
    """``filter_subband_3d_z`` of a (Z, Y, X) block with every step in float64; returns float64."""
    filters = D.db_filters(9)
    x = np.log1p(np.asarray(bl, dtype=np.float64))
    out = np.empty_like(x)
    for y in range(x.shape[1]):
        out[:, y, :] = _slice_f64(x[:, y, :].T, sigma, levels, filters).T
    return np.expm1(out)


# ----------------------------------------------------------------------------------------------------------------- volumes
def striped(shape, seed, stripes=True):
    """Uniform [0.5, 0.7), every 7th column of x times 1.5."""
    rng = np.random.default_rng(seed)
    v = (rng.random(shape) * 0.2 + 0.5).astype(np.float32)
    if stripes:
        gain = np.ones(shape[2], np.float32)
        gain[::7] = 1.5
        v = v * gain[None, None, :]
    return v


def striped_with_zeros(shape, seed):
    """Uniform [0, 1) times the every-7th-column gain 1.5, 30 % of the voxels exactly 0 (background: log1p(0) = 0 meets the zero
    padding)."""
    rng = np.random.default_rng(seed)
    v = rng.random(shape).astype(np.float32)
    gain = np.ones(shape[2], np.float32)
    gain[::7] = 1.5
    v = v * gain[None, None, :]
    v[rng.random(shape) < 0.3] = 0.0
    return v


# ------------------------------------------------------------------------------------------------------------------- cases
# id -> shape (Z, Y, X), sigma, explicit levels (0: wmaxlev), expected level count, builder, factor on TOL in the output domain
# (5 for the sigma = 60 cases, like the wide-notch assertion of test_destripe_explicit_levels_wide_notch_and_identity), and
# whether the log-domain comparison applies
def _case(shape, nlev, sigma=2.0, levels=0, build="striped", tol_factor=1, log_domain=True):
    return dict(shape=shape, sigma=sigma, levels=levels, nlev=nlev, build=build, tol_factor=tol_factor, log_domain=log_domain)


CASES = {
    "wide_even": _case((36, 1, 2100), 1),
    "wide_odd": _case((36, 2, 2101), 1),
    "two_tiles": _case((36, 1, 1030), 1, sigma=3.0),
    "deep3": _case((140, 1, 139), 3),
    "deep4": _case((272, 2, 276), 4),
    "odd_wide_notch": _case((74, 2, 68), 2, sigma=60.0, tol_factor=5),
    "odd_wide_notch_b": _case((70, 3, 68), 2, sigma=60.0, tol_factor=5),
    "tall": _case((600, 1, 40), 1),
    "zeros": _case((72, 2, 136), 2, build="striped_with_zeros", log_domain=False),
    "zeros_wide": _case((36, 1, 2100), 1, build="striped_with_zeros", log_domain=False),
    # log domain only while the reference's minimum stays above -0.5 (decided from the reference in the test)
    "over_levels": _case((40, 2, 64), 3, levels=3),
    # both extents below the 17 samples of the extension, explicit levels: 2 i + 1 - t = -16 reflects twice at level 1
    "multi_reflect": _case((12, 2, 20), 2, levels=2),
    # extents below lf - 1 = 17 with explicit levels: the coefficient counts GROW from level to level (12 -> 14 -> 15 -> 16), so
    # level 1 is not the largest user of the scratch that the levels share; the second with a notch of several bins, whose
    # sum is kept in that scratch
    "growing": _case((12, 2, 12), 3, levels=3),
    "growing_notch": _case((12, 2, 12), 2, sigma=8.0, levels=2, tol_factor=5),
    # the two volumes of the unaligned-base test (cols % 4 == 0), here at offset 0
    "base_1level": _case((40, 3, 64), 1),
    "base_2level": _case((72, 2, 136), 2),
}
WIDE = ("wide_even", "wide_odd", "zeros_wide")
SEED = 31
_BUILDERS = {"striped": striped, "striped_with_zeros": striped_with_zeros}


@functools.lru_cache(maxsize=None)
def reference(case_id):
    """(volume float32, float32 oracle, float64 reference) of a case, computed once per process; treat them as read-only."""
    c = CASES[case_id]
    vol = _BUILDERS[c["build"]](c["shape"], SEED)
    ref32 = D.filter_subband_3d_z(vol, c["sigma"], c["levels"])
    ref64 = filter_subband_3d_z_f64(vol, c["sigma"], c["levels"])
    for a in (vol, ref32, ref64):
        a.setflags(write=False)
    return vol, ref32, ref64


def log_distance(a, b):
    """max |log1p(a) - log1p(b)| in float64"""
    return float(np.abs(np.log1p(np.asarray(a, np.float64)) - np.log1p(np.asarray(b, np.float64))).max())


# -------------------------------------------------------------------------------------------- launch geometry, restated
def coefficient_counts(n, levels):
    """[n_1, .., n_levels]: floor((n + lf - 1) / 2) per level, from the even-padded extent n."""
    out = []
    for _ in range(levels):
        n = (n + LF - 1) // 2
        out.append(n)
    return out


def x_analysis_tiles(nx):
    """(tiles, interior segments) of k_dwt_x at level 1 of a block nx wide."""
    px = nx + nx % 2
    m = (px + LF - 1) // 2
    tiles = (m + K_TILE_A - 1) // K_TILE_A
    interior = sum(1 for t in range(tiles) if 2 * t * K_TILE_A - 16 >= 0 and 2 * t * K_TILE_A - 16 + SEGMENT <= nx)
    return tiles, interior


def x_synthesis_tiles(nx):
    px = nx + nx % 2
    return ((px + 1) // 2 + K_TILE_X - 1) // K_TILE_X


def z_chunk_grid(columns, steps):
    """(chunk length, chunks launched) of the column kernels: z_chunks() of destripe.hip and the grid made from it."""
    want = 256 * 2048
    c = 1 if columns >= want else (want + columns - 1) // columns
    zc = min(c, max(1, steps // 16))
    chunk = (steps + zc - 1) // zc
    return chunk, (steps + chunk - 1) // chunk


# ------------------------------------------------------------------------------------------------------- guarded buffers
def guarded(vol, dev, guard=64, offset=0):
    """(buf, view): ``buf`` a flat float32 device tensor [guard | offset | vol.size | guard] filled with SENTINEL, ``view`` the
    contiguous part of it that holds ``vol``, starting 4 * offset bytes past a 16-byte boundary."""
    import torch
    n = int(vol.size)
    buf = torch.full((guard + offset + n + guard,), SENTINEL, dtype=torch.float32, device=dev)
    view = buf[guard + offset:guard + offset + n].view(tuple(vol.shape))
    view.copy_(torch.from_numpy(np.ascontiguousarray(vol, dtype=np.float32)))
    assert view.is_contiguous() and view.data_ptr() % 16 == (4 * offset) % 16, (view.data_ptr() % 16, offset)
    return buf, view


def assert_guards_intact(buf, view):
    """Every element of ``buf`` outside ``view`` still equals SENTINEL (a NaN written there compares unequal, so it is seen)."""
    start = (view.data_ptr() - buf.data_ptr()) // 4
    flat = buf.cpu().numpy()
    front, back = flat[:start], flat[start + view.numel():]
    assert front.size > 0 and back.size > 0
    bad = np.flatnonzero(~(front == np.float32(SENTINEL)))
    assert bad.size == 0, f"{bad.size} element(s) written in front of the view, the nearest {start - int(bad[-1])} before it"
    bad = np.flatnonzero(~(back == np.float32(SENTINEL)))
    assert bad.size == 0, f"{bad.size} element(s) written behind the view, the nearest {int(bad[0])} past its end"
