"""TEST INFRASTRUCTURE for channel alignment (tests/test_channel_align_host.py, tests/test_gpu_channel_align.py).

OpenCV and scikit-image are installed on neither machine, so the yardstick is a numpy restatement written from their description
(DESIGN section 18).  Images are float32 and every per-pixel operation is a separate float32 operation in a fixed order, so the
per-pixel values are the device's bit for bit; sums are float64.

* sobel: ``h`` and ``v`` are the convolutions with ``[1, 0, -1]`` across and ``[1, 2, 1]`` along, over 8, border ``reflect``
  (d c b a | a b c d), accumulated in float64 in the order written in ``sobel`` and rounded to float32; ``sqrt((h*h + v*v) / 2)``.
* blur: taps ``[1, 4, 6, 4, 1] / 16`` along rows, then along columns, ``((((c1*a + c4*b) + c6*c) + c4*d) + c1*e)``, border
  REFLECT_101 (d c b | a b c d); gradients ``0.5 * next - 0.5 * previous`` with the same border.
* one ECC iteration at ``(tx, ty)``: ``ix = floor(tx)``, ``fx = float32(tx - ix)``, weights ``w00 = (1-fx)*(1-fy)``, ``w01 = fx*(1-fy)``,
  ``w10 = (1-fx)*fy``, ``w11 = fx*fy``; a sample is ``((w00*a + w01*b) + w10*c) + w11*d`` with zeros outside the plane; the mask is 1
  where ``(x + floor(tx + 0.5), y + floor(ty + 0.5))`` lies inside.  The sums and the step are those of ``ecc_step``.
"""
from __future__ import annotations

import math
import struct
import zlib

import numpy as np

F = np.float32
SUM_NAMES = ("n", "sw", "sww", "st", "stt", "swt", "hxx", "hxy", "hyy", "gxw", "gyw", "mgx", "mgy", "gxt", "gyt")
ECC_OK, ECC_NAN, ECC_MINIMIZED = 0, 1, 2


# ---------------------------------------------------------------------------------------------------------------------------------
# sobel, blur, gradients

def sobel(img):
    a = np.pad(np.asarray(img, F).astype(np.float64), 1, mode="symmetric")   # numpy's symmetric is scipy's reflect
    ny, nx = img.shape

    def p(dy, dx):
        return a[1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    h = (((((0.125 * p(1, -1) + 0.25 * p(1, 0)) + 0.125 * p(1, 1)) - 0.125 * p(-1, -1)) - 0.25 * p(-1, 0)) - 0.125 * p(-1, 1)).astype(F)
    v = (((((0.125 * p(-1, 1) + 0.25 * p(0, 1)) + 0.125 * p(1, 1)) - 0.125 * p(-1, -1)) - 0.25 * p(0, -1)) - 0.125 * p(1, -1)).astype(F)
    return np.sqrt((h * h + v * v) / F(2))


def _taps5(a, b, c, d, e):
    return (((F(0.0625) * a + F(0.25) * b) + F(0.375) * c) + F(0.25) * d) + F(0.0625) * e


def blur5(img):
    img = np.asarray(img, F)
    ny, nx = img.shape
    a = np.pad(img, ((0, 0), (2, 2)), mode="reflect")   # numpy's reflect is REFLECT_101
    rows = _taps5(*(a[:, k:k + nx] for k in range(5)))
    b = np.pad(rows, ((2, 2), (0, 0)), mode="reflect")
    return _taps5(*(b[k:k + ny, :] for k in range(5)))


def gradients(s):
    s = np.asarray(s, F)
    ny, nx = s.shape
    a = np.pad(s, ((0, 0), (1, 1)), mode="reflect")
    b = np.pad(s, ((1, 1), (0, 0)), mode="reflect")
    return F(0.5) * a[:, 2:] - F(0.5) * a[:, :nx], F(0.5) * b[2:, :] - F(0.5) * b[:ny, :]


def ecc_prepare(tmpl, subj):
    s = blur5(subj)
    gx, gy = gradients(s)
    return blur5(tmpl), s, gx, gy


# ---------------------------------------------------------------------------------------------------------------------------------
# one ECC iteration

def _shifted(a, iy, ix):
    """out[y, x] = a[y + iy, x + ix], zero outside"""
    ny, nx = a.shape
    out = np.zeros_like(a)
    y0, y1 = max(0, -iy), min(ny, ny - iy)
    x0, x1 = max(0, -ix), min(nx, nx - ix)
    if y0 < y1 and x0 < x1:
        out[y0:y1, x0:x1] = a[y0 + iy:y1 + iy, x0 + ix:x1 + ix]
    return out


def warp(a, tx, ty):
    ix, iy = math.floor(tx), math.floor(ty)
    fx, fy = F(tx - ix), F(ty - iy)
    one = F(1)
    w00, w01, w10, w11 = (one - fx) * (one - fy), fx * (one - fy), (one - fx) * fy, fx * fy
    return ((w00 * _shifted(a, iy, ix) + w01 * _shifted(a, iy, ix + 1)) + w10 * _shifted(a, iy + 1, ix)) + w11 * _shifted(a, iy + 1, ix + 1)


def mask(shape, tx, ty):
    return _shifted(np.ones(shape, F), math.floor(ty + 0.5), math.floor(tx + 0.5)) > 0


def ecc_terms(planes, tx, ty):
    """per-pixel float64 terms of every sum: dict name -> array (products of float32 values, exact)"""
    t, s, gx, gy = planes
    w, gxw, gyw = (warp(p, tx, ty).astype(np.float64) for p in (s, gx, gy))
    m = mask(t.shape, tx, ty).astype(np.float64)
    t = t.astype(np.float64)
    return {"n": m, "sw": m * w, "sww": m * (w * w), "st": m * t, "stt": m * (t * t), "swt": m * (w * t), "hxx": gxw * gxw, "hxy": gxw * gyw,
            "hyy": gyw * gyw, "gxw": gxw * w, "gyw": gyw * w, "mgx": m * gxw, "mgy": m * gyw, "gxt": m * (gxw * t), "gyt": m * (gyw * t)}


def ecc_sums(planes, tx, ty):
    """(sums, sums of absolute terms): float64 arrays in SUM_NAMES order"""
    terms = ecc_terms(planes, tx, ty)
    return (np.array([math.fsum(terms[k].ravel()) for k in SUM_NAMES]), np.array([math.fsum(np.abs(terms[k]).ravel()) for k in SUM_NAMES]))


def derived(S):
    """the quantities of the step from the factored sums"""
    S = dict(zip(SUM_NAMES, S))
    with np.errstate(all="ignore"):
        n = np.float64(S["n"])
        mean_w, mean_t = S["sw"] / n, S["st"] / n
        return {"wn2": max(S["sww"] - S["sw"] * mean_w, 0.0) if n else np.nan, "tn2": max(S["stt"] - S["st"] * mean_t, 0.0) if n else np.nan,
                "corr": S["swt"] - S["sw"] * mean_t, "ipx": S["gxw"] - mean_w * S["mgx"], "ipy": S["gyw"] - mean_w * S["mgy"],
                "tpx": S["gxt"] - mean_t * S["mgx"], "tpy": S["gyt"] - mean_t * S["mgy"], "hxx": S["hxx"], "hxy": S["hxy"], "hyy": S["hyy"]}


def derived_two_pass(planes, tx, ty):
    """the same quantities the way OpenCV takes them: subtract the means inside the mask, then multiply and sum"""
    t, s, gx, gy = planes
    w, gxw, gyw = (warp(p, tx, ty).astype(np.float64) for p in (s, gx, gy))
    m = mask(t.shape, tx, ty)
    t = t.astype(np.float64)
    w_zm = np.where(m, w - w[m].mean(), w)
    t_zm = np.where(m, t - t[m].mean(), 0.0)
    f = lambda a: math.fsum(a.ravel())   # noqa: E731
    return {"wn2": f(w_zm[m] ** 2), "tn2": f(t_zm[m] ** 2), "corr": f(t_zm * w_zm), "ipx": f(gxw * w_zm), "ipy": f(gyw * w_zm), "tpx": f(gxw * t_zm),
            "tpy": f(gyw * t_zm), "hxx": f(gxw * gxw), "hxy": f(gxw * gyw), "hyy": f(gyw * gyw)}


def natural_scale(name, d):
    """What a derived quantity is measured against: a norm is its own scale, a correlation or a projection (sums with cancellation)
    the product of the norms of its two factors (Cauchy-Schwarz)."""
    if name in ("wn2", "tn2", "hxx", "hyy"):
        return abs(d[name])
    if name == "corr":
        return math.sqrt(d["wn2"] * d["tn2"])
    if name == "hxy":
        return math.sqrt(d["hxx"] * d["hyy"])
    return math.sqrt((d["hxx"] if name[2] == "x" else d["hyy"]) * (d["tn2"] if name[0] == "t" else d["wn2"]))


def ecc_step(S):
    """(rho, dtx, dty, status) of one iteration from its sums"""
    d = derived(S)
    with np.errstate(all="ignore"):
        rho = np.float64(d["corr"]) / (np.sqrt(np.float64(d["wn2"])) * np.sqrt(np.float64(d["tn2"])))
    if rho != rho:
        return rho, 0.0, 0.0, ECC_NAN
    det = d["hxx"] * d["hyy"] - d["hxy"] * d["hxy"]
    ixx, ixy, iyy = (d["hyy"] / det, -d["hxy"] / det, d["hxx"] / det) if det != 0 else (0.0, 0.0, 0.0)
    hix, hiy = ixx * d["ipx"] + ixy * d["ipy"], ixy * d["ipx"] + iyy * d["ipy"]
    lambda_n = d["wn2"] - (d["ipx"] * hix + d["ipy"] * hiy)
    lambda_d = d["corr"] - (d["tpx"] * hix + d["tpy"] * hiy)
    if not lambda_d > 0:
        return rho, 0.0, 0.0, ECC_MINIMIZED
    lam = lambda_n / lambda_d
    ex, ey = lam * d["tpx"] - d["ipx"], lam * d["tpy"] - d["ipy"]
    return rho, ixx * ex + ixy * ey, ixy * ex + iyy * ey, ECC_OK


def ecc_translation(tmpl, subj, iterations=10000, eps=1e-10):
    """findTransformECC's loop: (tx, ty, rho, iterations done, status)"""
    planes = ecc_prepare(tmpl, subj)
    tx = ty = 0.0
    rho, last = -1.0, -eps
    i = 0
    while i < iterations and abs(rho - last) >= eps:
        S = np.array([terms.sum() for terms in ecc_terms(planes, tx, ty).values()])
        last = rho
        rho, dx, dy, status = ecc_step(S)
        i += 1
        if status != ECC_OK:
            return tx, ty, rho, i, status
        tx, ty = tx + dx, ty + dy
    return tx, ty, rho, i, ECC_OK


class EccFailure(RuntimeError):
    pass


def get_gradient(img):
    return sobel(np.asarray(img).astype(F))


ITERATIONS = []   # the iteration count of every get_transformation_matrix call, for the fixture generator to look at


def get_transformation_matrix(reference, subject, iterations=10000, termination=1e-10):
    tx, ty, _, count, status = ecc_translation(reference, subject, iterations, termination)
    ITERATIONS.append(count)
    if status != ECC_OK:
        raise EccFailure(status)
    warp_matrix = np.eye(2, 3, dtype=F)
    warp_matrix[0, 2], warp_matrix[1, 2] = tx, ty
    return np.linalg.inv(np.append(warp_matrix, np.array([[0, 0, 1]], dtype=F), axis=0))


def block_reduce_mean(plane, factor):
    ny, nx = plane.shape
    padded = np.zeros((ny + -ny % factor, nx + -nx % factor), np.float64)
    padded[:ny, :nx] = plane
    return padded.reshape(padded.shape[0] // factor, factor, padded.shape[1] // factor, factor).mean(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------------------------------------
# the literal numpy steps of align_images.py

def pad_to_shape(pad_shape, arr):
    pad_dim = [pad_shape[i] - arr.shape[i] for i in range(len(pad_shape))]
    return np.pad(arr, [(x // 2, (x + 1) // 2) for x in pad_dim], mode="constant")


def trim_to_shape(output_shape, arr):
    trim = [arr.shape[i] - output_shape[i] for i in range(len(output_shape))]
    return arr[tuple(slice(x // 2, arr.shape[i] - (x + 1) // 2) for i, x in enumerate(trim))]


def roll_pad(arr, move, axis=0):
    """in place; a move of the extent or more leaves zeros"""
    if move == 0:
        return
    v = np.moveaxis(arr, axis, 0)
    rolled = np.zeros_like(v)
    n = v.shape[0]
    if 0 < move < n:
        rolled[move:] = v[:-move]
    elif -n < move < 0:
        rolled[:move] = v[-move:]
    v[...] = rolled


def get_layer(index, image, plane):
    """align_images.get_layer for a zyx volume: every plane comes out transposed"""
    if plane == "xy":
        return image[index, :, :].T
    return image[:, index, :].T if plane == "xz" else image[:, :, index].T


def composite_slice(n_ref, volumes, reference_index, offsets, out_dtype):
    """process_single_big_image for one output slice, step by step: [ny, nx, 3] of out_dtype.  volumes: [nz, ny, nx] or None per
    channel; offsets (z, y, x) per channel."""
    shapes = [None if v is None else v.shape for v in volumes]
    op = [max(d) for d in zip(*[s for s in shapes if s is not None])]
    pad_z = [None if s is None else (op[0] - s[0]) // 2 for s in shapes]
    ref_shape = shapes[reference_index][1:]
    planes = []
    for c, v in enumerate(volumes):
        if v is None:
            planes.append(np.zeros(ref_shape))
            continue
        n_img = n_ref if c == reference_index else n_ref + pad_z[reference_index] - pad_z[c] - offsets[c][0]
        if 0 <= n_img < shapes[c][0]:
            f = pad_to_shape(op[1:], v[n_img].copy())
            roll_pad(f, offsets[c][1], axis=0)
            roll_pad(f, offsets[c][2], axis=1)
            planes.append(trim_to_shape(ref_shape, f))
        else:
            planes.append(np.zeros(ref_shape))
    stacked = np.stack(planes, axis=-1)
    # the zeros of an absent slice make the stack float64; the samples are integers, and astype wraps them as it wraps integers
    return stacked.astype(np.int64).astype(out_dtype)


def composite(volumes, reference_index, offsets, out_dtype):
    return np.stack([composite_slice(n, volumes, reference_index, offsets, out_dtype) for n in range(volumes[reference_index].shape[0])])


def align_images(img1, img2, max_iter=50):
    """the outer loop of align_images.align_images on numpy volumes (img2 is moved): (x_moves, y_moves, z_moves, residual, sums) with
    ``sums`` the pre-rounding sums a + b of every outer iteration in x, y, z order"""
    x_moves, y_moves, z_moves, sums, prev = [], [], [], [], []
    residual, found, iteration = None, False, 0
    while iteration < max_iter:
        mats = {}
        for plane, idx in (("xy", img1.shape[0] // 2), ("xz", img1.shape[1] // 2), ("yz", img1.shape[2] // 2)):
            a, b = get_gradient(get_layer(idx, img1, plane)), get_gradient(get_layer(idx, img2, plane))
            mats[plane] = get_transformation_matrix(a, b)
        xy, xz, yz = mats["xy"], mats["xz"], mats["yz"]
        sums.append((float(xy[1][2] + xz[1][2]), float(xy[0][2] + yz[1][2]), float(xz[0][2] + yz[0][2])))
        x_moves.append(int(round(xy[1][2] + xz[1][2]) / 2))
        y_moves.append(int(round(xy[0][2] + yz[1][2]) / 2))
        z_moves.append(int(round(xz[0][2] + yz[0][2]) / 2))
        roll_pad(img2, x_moves[-1], axis=2)
        roll_pad(img2, y_moves[-1], axis=1)
        roll_pad(img2, z_moves[-1], axis=0)
        matr = [(int(xy[0][2]), int(xy[1][2])), (int(xz[0][2]), int(xz[1][2])), (int(yz[0][2]), int(yz[1][2]))]
        found = found or matr in prev
        if found or (x_moves[-1] == 0 and y_moves[-1] == 0 and z_moves[-1] == 0):
            residual = ((xy[0][2] + xz[0][2]) / 2, (xy[1][2] + yz[1][2]) / 2, (xz[1][2] + yz[0][2]) / 2)
            break
        prev.append(matr)
        iteration += 1
    return x_moves, y_moves, z_moves, residual, sums


def alignments_text(channels, input_files, residuals, reference):
    """the text of alignments.txt, written out line by line from the layout"""
    lines = [f"Number of channels: {len(channels)}\n"] + [f"\t Channel {i}: {input_files[i]}\n" for i in range(len(channels))]
    lines.append(f"Reference channel: {reference}\n")
    index = 0
    for n in range(len(channels) + 1):
        if n == reference:
            continue
        lines.append(f"Channel {n}:\n")
        for k, axis in enumerate("xyz"):
            tail = f"\t\t Residuals: {residuals[index][k]}" if residuals[index] is not None else ""
            lines.append(f"\t{axis}-alignment: {channels[index][k]}{tail}\n")
        lines[-1] += "\n"
        index += 1
    return "".join(lines)


# ---------------------------------------------------------------------------------------------------------------------------------
# synthetic data

def smooth_plane(shape, seed=3, blobs=24):
    """a smooth float32 plane of Gaussian blobs, as a function that can be sampled at a sub-pixel shift: returns f(dx, dy) -> plane
    with f(dx, dy)[y, x] = scene(x + dx, y + dy)"""
    rng = np.random.default_rng(seed)
    ny, nx = shape
    cy, cx = rng.uniform(0, ny, blobs), rng.uniform(0, nx, blobs)
    sig = rng.uniform(0.06, 0.16, blobs) * min(ny, nx) + 1.0
    amp = rng.uniform(50, 200, blobs)

    def at(dx=0.0, dy=0.0):
        y, x = np.mgrid[0:ny, 0:nx].astype(np.float64)
        out = np.full(shape, 10.0)
        for k in range(blobs):
            out += amp[k] * np.exp(-((y + dy - cy[k]) ** 2 + (x + dx - cx[k]) ** 2) / (2 * sig[k] ** 2))
        return out.astype(F)
    return at


def blob_volume(shape=(40, 48, 56), seed=5, blobs=60):
    """(reference, subject) uint16 volumes: Gaussian blobs plus noise; the subject is the reference rolled by (z, y, x) = (1, -2, 3),
    scaled by 0.6, plus an offset"""
    rng = np.random.default_rng(seed)
    nz, ny, nx = shape
    z, y, x = np.mgrid[0:nz, 0:ny, 0:nx].astype(np.float64)
    vol = np.zeros(shape)
    for _ in range(blobs):
        c = rng.uniform(0, 1, 3) * shape
        s = rng.uniform(1.5, 4.0)
        vol += rng.uniform(500, 4000) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    ref = np.clip(vol + 200 + rng.normal(0, 12, shape), 0, 65535).astype(np.uint16)
    moved = np.roll(vol, (1, -2, 3), axis=(0, 1, 2))
    sub = np.clip(0.6 * moved + 150 + rng.normal(0, 12, shape), 0, 65535).astype(np.uint16)
    return ref, sub


ECC_CASES = {   # plane shape -> (seed of smooth_plane, the shift (dx, dy) of the subject's scene; the truth is tx = -dx, ty = -dy)
    (9, 11): (4, (0.5, -0.25)),
    (37, 53): (3, (2.3, -1.7)),
    (64, 64): (3, (0.5, -0.25)),
    (131, 257): (3, (-6.0, 4.0)),
}


def ecc_case(shape):
    """(template, subject, truth (tx, ty)) of a plane shape"""
    seed, (dx, dy) = ECC_CASES[tuple(shape)]
    at = smooth_plane(tuple(shape), seed)
    return at(), at(dx, dy), (-dx, -dy)


def half_integer_margin(sums):
    """smallest distance of any pre-rounding sum to a half-integer: Python's round flips there"""
    return min(abs((s - 0.5) - round(s - 0.5)) for triple in sums for s in triple)


def main_fixture(seed=11):
    """three channels for main(): down-sampled stacks of shapes that differ by odd amounts and full-resolution slices at twice the
    y / x sampling (uint16): (down [3 volumes], orig [3 volumes]).  Green is red moved by (z, y, x) = (0, -2, 3), blue by (1, 2, -1)."""
    rng = np.random.default_rng(seed)
    shape = (12, 48, 64)
    z, y, x = np.mgrid[0:12, 0:48, 0:64].astype(np.float64)
    vol = np.zeros(shape)
    for _ in range(40):
        c = rng.uniform(0.2, 0.8, 3) * shape   # away from the faces: numpy.roll wraps, and 12 slices leave little room
        s = rng.uniform(1.5, 3.0)
        vol += rng.uniform(500, 4000) * np.exp(-((z - c[0]) ** 2 + (y - c[1]) ** 2 + (x - c[2]) ** 2) / (2 * s * s))
    down, orig = [], []
    for move, gain, base, trimmed in (((0, 0, 0), 1.0, 200, (12, 48, 64)), ((0, -2, 3), 0.6, 150, (12, 47, 64)), ((1, 2, -1), 0.8, 100, (11, 48, 61))):
        v = np.clip(gain * np.roll(vol, move, axis=(0, 1, 2)) + base + rng.normal(0, 2, shape), 0, 65535).astype(np.uint16)
        d = np.ascontiguousarray(trim_to_shape(trimmed, v))
        down.append(d)
        orig.append(np.ascontiguousarray(np.repeat(np.repeat(d, 2, axis=1), 2, axis=2)))
    return down, orig


def main_expected(down, orig, reference, max_iter, dtype, dx, dy, dz):
    """align_images.main on numpy volumes, line by line with its quirks: dict with ``alignments`` (x, y, z per channel), ``residuals``,
    ``sums`` (per aligned channel), ``scaled`` (z, y, x per channel), ``down_rgb`` and ``orig_rgb`` [n, ny, nx, 3]"""
    ref_shape = down[reference].shape
    op = tuple(max(d) for d in zip(*[v.shape for v in down if v is not None]))
    channels = [None if v is None else pad_to_shape(op, v) for v in down]
    copies = [None if v is None else v.copy() for v in channels]
    alignments, residuals, sums = [], [], {}
    for i, v in enumerate(copies):
        if v is None or i == reference:
            alignments.append([None, None, None])
            residuals.append(None)
            continue
        xs, ys, zs, res, pre = align_images(copies[reference], v, max_iter)
        alignments.append([sum(xs), sum(ys), sum(zs)])
        residuals.append(res)
        sums[i] = pre
    arrays = main_arrays(down, orig, reference, alignments, dtype, dx, dy, dz)
    return {"alignments": alignments, "residuals": residuals, "sums": sums, **arrays}


def main_arrays(down, orig, reference, alignments, dtype, dx, dy, dz):
    """what main() writes, given the alignments: ``down_rgb`` (dtype), ``orig_rgb`` (the reference slices' dtype), ``scaled``"""
    ref_shape = down[reference].shape
    op = tuple(max(d) for d in zip(*[v.shape for v in down if v is not None]))
    channels = [None if v is None else pad_to_shape(op, v) for v in down]
    for n in range(len(channels)):   # kept: index 0 is skipped whatever the reference is, and the trim sits inside the loop
        if not n or n == reference:
            continue
        if channels[n] is not None:
            roll_pad(channels[n], alignments[n][0], axis=2)
            roll_pad(channels[n], alignments[n][1], axis=1)
            roll_pad(channels[n], alignments[n][2], axis=0)
        for m in range(len(channels)):
            if channels[m] is not None:
                channels[m] = trim_to_shape(ref_shape, channels[m])
    layers = [np.zeros_like(channels[reference]) if v is None else v for v in channels]
    down_rgb = np.stack(layers, axis=-1).astype(dtype)
    ratios = [float(o) / d for o, d in (dx, dy, dz)]
    scaled = [[0, 0, 0] if n == reference or alignments[n][0] is None else [int(alignments[n][i] / ratios[i]) for i in (2, 1, 0)]
              for n in range(len(orig))]
    return {"scaled": scaled, "down_rgb": down_rgb, "orig_rgb": composite(orig, reference, scaled, orig[reference].dtype)}


COMPOSITE_CASES = {   # name -> (channel shapes, reference, offsets (z, y, x) per channel)
    "odd-differences": ([(6, 9, 12), (5, 12, 11), (9, 10, 15)], 0, [[0, 0, 0], [1, -2, 3], [-2, 4, -1]]),
    "reference-in-the-middle": ([(6, 9, 12), (5, 12, 11), (9, 10, 15)], 1, [[2, 1, -5], [0, 0, 0], [-1, 0, 2]]),
    "larger-than-the-extent": ([(4, 8, 9), (4, 8, 9), (4, 7, 9)], 0, [[0, 0, 0], [0, 30, 0], [0, 0, -40]]),
    "absent-channel": ([(4, 8, 9), None, (5, 7, 12)], 2, [[1, 2, -1], [0, 0, 0], [0, 0, 0]]),
    "slices-out-of-range-at-both-ends": ([(6, 5, 6), (6, 5, 6), (3, 5, 6)], 0, [[0, 0, 0], [4, 0, 1], [-3, -1, 0]]),
}


def composite_volumes(shapes, dtype, seed=6):
    rng = np.random.default_rng(seed)
    top = 250 if np.dtype(dtype) == np.uint8 else 65000
    return [None if s is None else rng.integers(1, top, s).astype(dtype) for s in shapes]


# ---------------------------------------------------------------------------------------------------------------------------------
# a small reader of the RGB files (classic little-endian TIFF, strips, chunky, none / Adobe deflate)

def read_tiff(path):
    """(array [ny, nx, samples] or [ny, nx], tags dict)"""
    data = open(path, "rb").read()
    assert data[:4] == b"II*\0", "classic little-endian TIFF expected"
    (ifd,) = struct.unpack_from("<I", data, 4)
    (count,) = struct.unpack_from("<H", data, ifd)
    tags = {}
    for k in range(count):
        tag, typ, n, _ = struct.unpack_from("<HHII", data, ifd + 2 + 12 * k)
        size, code = {3: (2, "H"), 4: (4, "I")}[typ]
        at = ifd + 2 + 12 * k + 8
        if size * n > 4:
            (at,) = struct.unpack_from("<I", data, at)
        tags[tag] = list(struct.unpack_from(f"<{n}{code}", data, at))
    assert struct.unpack_from("<I", data, ifd + 2 + 12 * count)[0] == 0
    nx, ny, spp = tags[256][0], tags[257][0], tags.get(277, [1])[0]
    bits, fmt = tags[258], tags.get(339, [1] * spp)
    assert len(set(bits)) == 1 and len(set(fmt)) == 1 and len(bits) == spp and tags.get(284, [1])[0] == 1
    dtype = {(8, 1): np.uint8, (16, 1): np.uint16, (32, 1): np.uint32, (32, 3): np.float32}[(bits[0], fmt[0])]
    raw = b""
    for off, cnt in zip(tags[273], tags[279]):
        strip = data[off:off + cnt]
        raw += zlib.decompress(strip) if tags[259][0] == 8 else strip
    arr = np.frombuffer(raw, dtype).reshape((ny, nx, spp) if spp > 1 else (ny, nx))
    return arr, tags
