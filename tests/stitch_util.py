"""A numpy restatement of stitching step 6 (``terastitcher -6``, resolution 0), the yardstick of ``mi_merge_slab``.

It transliterates the loops of the reference, for the whole volume (every row and column of stacks):

  volume_dims          StackStitcher::computeVolumeDims (StackStitcher.cpp:405-560): V/H union, the shared D range
  stripe               StackStitcher::getStripe2 (StackStitcher.cpp:1854-2140): one row of stacks, blended across H
  merge_slice          UnstitchedVolume::internal_loadSubvolume_to_real32 (UnstitchedVolume.cpp:412-899): stripes blended
                       across V column by column, between the corners of the two stripes
  sinusoidal / no_blending   StackStitcher.h:127-138
  to_samples           uint16(v * 65535.0F) / uint8(v * 255.0f) (UnstitchedVolume.cpp:1086-1198)

Reads that the reference makes past the end of a stripe row (the non-overlapping copy compares against the absolute right edge,
UnstitchedVolume.cpp:879) land on the next row of the same buffer, as there; reads past the whole buffer give 0.
It is checked against the binary's own output in tests/test_stitch_placement.py.
"""
from __future__ import annotations

import math

import numpy as np

PI = 3.14159265          # IM_config.h:149, volumemanager.config.h:94
S_PI = 3.14159265        # S_config.h:48
SINBLEND, NOBLEND = 0, 1


def volume_dims(abs_v, abs_h, abs_d, height, width, n_slices):
    """(V0, V1, H0, H1, D0, D1) of the stitched volume in the stacks' absolute frame."""
    abs_v, abs_h, abs_d = (np.asarray(a) for a in (abs_v, abs_h, abs_d))
    V0 = int(abs_v[0].min())
    V1 = int(abs_v[-1].max()) + height
    H0 = int(abs_h[:, 0].min())
    H1 = int(abs_h[:, -1].max()) + width
    D0 = int(abs_d.max())
    D1 = int(abs_d.min()) + n_slices
    return V0, V1, H0, H1, D0, D1


def sinusoidal(angle, p1, p2):
    """Elementwise over arrays p1, p2 (float32) for one angle."""
    w = (math.cos(angle) + 1.0) * 0.5 if math.isfinite(angle) else math.nan
    out = (w * p1.astype(np.float64) + (1.0 - w) * p2.astype(np.float64)).astype(np.float32)
    black = (p1 == 0) | (p2 == 0)
    return np.where(black, np.maximum(p1, p2), out)


def no_blending(angle, p1, p2):
    return p1.copy() if angle <= S_PI / 2 else p2.copy()


def _blend_rows(blending, angles, p1, p2):
    """The blend of one column of an overlap, every row at its own angle."""
    if blending == NOBLEND:
        return np.where(angles <= S_PI / 2, p1, p2)
    with np.errstate(invalid="ignore"):
        w = (np.cos(angles) + 1.0) * 0.5
    out = (w * p1.astype(np.float64) + (1.0 - w) * p2.astype(np.float64)).astype(np.float32)
    return np.where((p1 == 0) | (p2 == 0), np.maximum(p1, p2), out)


def _flat_read(buf, rows, col):
    """buf[rows, col] with the flat-buffer semantics of a C pointer walk: a column outside the row continues on the neighbouring
    row; positions outside the buffer read as 0."""
    h, w = buf.shape
    f = rows.astype(np.int64) * w + col
    ok = (f >= 0) & (f < h * w)
    out = np.zeros(rows.shape, np.float32)
    out[ok] = buf.reshape(-1)[f[ok]]
    return out


def stripe(tiles, r, abs_v, abs_h, height, width, blending):
    """getStripe2 for row r: ``tiles[r][c]`` are float32 (height, width) slices; returns (stripe, top, left)."""
    C = abs_v.shape[1]
    blend = sinusoidal if blending == SINBLEND else no_blending
    top = int(abs_v[r].min())
    bottom = int(abs_v[r].max()) + height
    left = int(abs_h[r, 0])
    right = int(abs_h[r, C - 1]) + width
    H, W = bottom - top, right - left
    out = np.zeros((H, W), np.float32)
    rows = np.arange(H)
    for c in range(C):
        l_ok = c > 0
        rr_ok = c < C - 1
        r_top = int(abs_v[r, c]) - top
        r_left = int(abs_h[r, c]) - left
        if l_ok:
            l_top = int(abs_v[r, c - 1]) - top
            l_left = int(abs_h[r, c - 1]) - left
            l_right = int(abs_h[r, c - 1]) - left + width
            delta = PI / ((int(abs_h[r, c - 1]) + width - int(abs_h[r, c])) - 1) if \
                (int(abs_h[r, c - 1]) + width - int(abs_h[r, c])) - 1 != 0 else math.inf
        rr_left = int(abs_h[r, c + 1]) - left if rr_ok else None
        angle = 0.0
        j_end = min(rr_left, r_left + width) if rr_ok else W
        rv = (rows - r_top >= 0) & (rows - r_top < height)
        for j in range(r_left if l_ok else 0, j_end):
            R = np.zeros(H, np.float32)
            R[rv] = tiles[r][c][rows[rv] - r_top, j - r_left]
            if l_ok and j < l_right:
                lv = (rows - l_top >= 0) & (rows - l_top < height)
                L = np.zeros(H, np.float32)
                L[lv] = tiles[r][c - 1][rows[lv] - l_top, j - l_left]
                both = rv & lv
                col = out[:, j]
                if both.any():
                    col[both] = blend(angle, L[both], R[both])
                col[rv & ~lv] = R[rv & ~lv]
                col[lv & ~rv] = L[lv & ~rv]
                angle = angle + delta
            else:
                out[rv, j] = R[rv]
    return out, top, left


def _corners(abs_v, abs_h, height, width):
    """stripesCorners (UnstitchedVolume.cpp:596-672): per row the (H, h, up) lists ``ups`` and ``bottoms``, with the reused
    ``tmp.h`` of the last corners."""
    R, C = abs_v.shape
    out = []
    for r in range(R):
        ul_v = int(abs_v[r].min())
        br_v = int(abs_v[r].max()) + height
        ups, bottoms = [], []
        tmp_h = int(abs_v[r, 0]) - ul_v
        ups.append((int(abs_h[r, 0]), tmp_h, True))
        tmp_h = br_v - int(abs_v[r, 0]) - height
        bottoms.append((int(abs_h[r, 0]), tmp_h, False))
        for c in range(C - 1):
            if abs_v[r, c] < abs_v[r, c + 1]:
                ups.append((int(abs_h[r, c]) + width, int(abs_v[r, c + 1]) - ul_v, True))
                tmp_h = br_v - int(abs_v[r, c + 1]) - height
                bottoms.append((int(abs_h[r, c + 1]), tmp_h, False))
            else:
                ups.append((int(abs_h[r, c + 1]), int(abs_v[r, c + 1]) - ul_v, True))
                tmp_h = br_v - int(abs_v[r, c + 1]) - height
                bottoms.append((int(abs_h[r, c]) + width, tmp_h, False))
        end = int(abs_h[r, C - 1]) + width
        ups.append((end, tmp_h, True))
        bottoms.append((end, tmp_h, False))
        out.append((ups, bottoms))
    return out


def merged_corners(abs_v, abs_h, height, width):
    """merged[r-1] = bottoms of row r-1 merged with ups of row r, by H, stable (std::list::merge, *this first on ties)."""
    cs = _corners(abs_v, abs_h, height, width)
    res = []
    for r in range(1, abs_v.shape[0]):
        a, b = cs[r - 1][1], cs[r][0]
        m, i, k = [], 0, 0
        while i < len(a) or k < len(b):
            if k >= len(b) or (i < len(a) and not (b[k][0] < a[i][0])):
                m.append(a[i])
                i += 1
            else:
                m.append(b[k])
                k += 1
        res.append(m)
    return res


def merge_slice(tiles, abs_v, abs_h, height, width, blending=SINBLEND):
    """One stitched slice (float32, (V1-V0, H1-H0)) from ``tiles[r][c]`` = the float32 slice of stack (r, c) at that depth."""
    abs_v, abs_h = np.asarray(abs_v), np.asarray(abs_h)
    R, C = abs_v.shape
    V0 = int(abs_v[0].min())
    V1 = int(abs_v[-1].max()) + height
    H0 = int(abs_h[:, 0].min())
    H1 = int(abs_h[:, -1].max()) + width
    Hh, Ww = V1 - V0, H1 - H0
    if R == 1 and C == 1:
        return tiles[0][0].astype(np.float32).copy()
    blend = sinusoidal if blending == SINBLEND else no_blending
    buf = np.zeros((Hh, Ww), np.float32)
    ul_v = [int(abs_v[r].min()) for r in range(R)]
    br_v = [int(abs_v[r].max()) + height for r in range(R)]
    ul_h = [int(abs_h[r, 0]) for r in range(R)]
    br_h = [int(abs_h[r, C - 1]) + width for r in range(R)]
    merged = merged_corners(abs_v, abs_h, height, width)
    up = None
    ov = 0
    for r in range(R):
        down, _, _ = stripe(tiles, r, abs_v, abs_h, height, width, blending)
        d_top = ul_v[r] - V0
        d_left = ul_h[r] - H0
        if up is not None:
            u_bottom = br_v[r - 1] - V0
            u_top = ul_v[r - 1] - V0
            u_left = ul_h[r - 1] - H0
            ov = u_bottom - d_top
        dd_top = ul_v[r + 1] - V0 if r != R - 1 else None
        h_up = h_down = ov
        if up is not None:
            m = merged[r - 1]
            for q in range(len(m) - 1):
                cl, cr = m[q], m[q + 1]
                if q + 2 == len(m):
                    h_up, h_down = (ov, 0) if cl[2] else (0, ov)
                elif cl[2]:
                    h_up = cl[1]
                else:
                    h_down = cl[1]
                h_ov = ov - h_up - h_down
                delta = PI / (h_ov - 1) if h_ov - 1 != 0 else math.inf
                for j in range(cl[0] - H0, cr[0] - H0):
                    a, b = d_top, min(d_top + h_up + (0 if h_ov >= 0 else h_ov), Hh)
                    if b > a:
                        rows = np.arange(a, b)
                        buf[a:b, j] = _flat_read(up, rows - u_top, j - u_left)
                    a, b = d_top + h_up, min(d_top + h_up + h_ov, Hh)
                    if b > a:
                        rows = np.arange(a, b)
                        p1 = _flat_read(up, rows - u_top, j - u_left)
                        p2 = _flat_read(down, rows - d_top, j - d_left)
                        # angle = angle + delta per row: a sequential running sum (np.add.accumulate adds in order)
                        angles = np.add.accumulate(np.concatenate([[0.0], np.full(b - a - 1, delta)]))
                        buf[a:b, j] = [blend(float(t), p1[q:q + 1], p2[q:q + 1])[0] for q, t in enumerate(angles)] \
                            if b - a < 4 else _blend_rows(blending, angles, p1, p2)
                    a, b = d_top + h_up + (h_ov if h_ov >= 0 else 0), d_top + h_up + h_ov + h_down
                    if b > a:
                        rows = np.arange(a, b)
                        buf[a:b, j] = _flat_read(down, rows - d_top, j - d_left)
        a = 0 if r == 0 else br_v[r - 1] - V0
        b = Hh if r == R - 1 else dd_top
        if b > a:
            js = np.arange(Ww)
            ok = (js - d_left >= 0) & (js - d_left < br_h[r])
            for i in range(a, b):
                buf[i, ok] = _flat_read(down, np.full(int(ok.sum()), i - d_top), js[ok] - d_left)
        up = down
    return buf


def to_samples(vol, dtype):
    """VolumeConverter's real32 -> integer conversion: truncation of v * 65535.0F (v * 255.0f)."""
    f = np.float32(65535.0) if np.dtype(dtype) == np.uint16 else np.float32(255.0)
    return (vol.astype(np.float32) * f).astype(dtype)


def to_float(samples):
    """loadImageStack's scaling (tiff2D.cpp:606-610): float32 sample / 65535 (/ 255)."""
    f = np.float32(65535.0) if samples.dtype == np.uint16 else np.float32(255.0)
    return samples.astype(np.float32) / f


def merge_volume(stacks, abs_v, abs_h, abs_d, blending=SINBLEND, D0=None, D1=None):
    """The stitched volume (integer samples, (D, V, H)) of ``stacks[r][c]`` = (n_slices, height, width) uint8/uint16 arrays;
    D0 / D1 select output slices of the stitched volume (0-based)."""
    abs_v, abs_h, abs_d = (np.asarray(a) for a in (abs_v, abs_h, abs_d))
    n, height, width = stacks[0][0].shape
    vd0, vd1 = int(abs_d.max()), int(abs_d.min()) + n
    depth = vd1 - vd0
    D0 = 0 if D0 is None else D0
    D1 = depth if D1 is None else D1
    out = []
    for z in range(D0, D1):
        tiles = [[to_float(stacks[r][c][z + vd0 - int(abs_d[r, c])]) for c in range(abs_v.shape[1])] for r in range(abs_v.shape[0])]
        out.append(to_samples(merge_slice(tiles, abs_v, abs_h, height, width, blending), stacks[0][0].dtype))
    return np.stack(out)
