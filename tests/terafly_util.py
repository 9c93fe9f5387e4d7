"""Numpy restatement of the reference's TeraFly conversion (``teraconverter --dfmt="TIFF (tiled, 3D)"`` from a 2-D series):
VolumeConverter::generateTilesVaa3DRaw's grouping, block and naming rules, VirtualVolume::halveSample_UINT8 /
halveSample2D_UINT8, and TiledVolume::save / Block::binarizeInto for mdata.bin.  Independent of ipp_amd.terafly; checked
against the binary's goldens (tests/golden/terafly) by tests/test_terafly_host.py."""
import hashlib
import math
import os
import struct

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "terafly")


def golden_runs():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f != "refused.npz")


def load_golden(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def golden_input(g):
    dtype, shape, seed = str(g["recipe_dtype"]), tuple(int(v) for v in g["recipe_shape"]), int(g["recipe_seed"])
    bits = np.dtype(dtype).itemsize * 8
    vol = np.random.default_rng(seed).integers(0, 2 ** bits, shape, dtype=dtype)
    assert hashlib.sha256(vol.tobytes()).hexdigest() == str(g["input_sha"]), "seeded generator drifted"
    return vol


def pages_sha(pages):
    return hashlib.sha256(np.ascontiguousarray(pages).tobytes()).hexdigest()


def halve3d(a, method):
    d, h, w = a.shape
    a = a[:d // 2 * 2, :h // 2 * 2, :w // 2 * 2]
    parts = [a[z::2, i::2, j::2] for z in (0, 1) for i in (0, 1) for j in (0, 1)]
    if method == "max":
        return np.maximum.reduce(parts).astype(a.dtype)
    s = np.sum([p.astype(np.int64) for p in parts], axis=0)
    return ((s + 4) >> 3).astype(a.dtype)          # iim::round(sum / 8.0f): half away from zero, exact in float


def halve2d(a, method):
    d, h, w = a.shape
    a = a[:, :h // 2 * 2, :w // 2 * 2]
    parts = [a[:, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    if method == "max":
        return np.maximum.reduce(parts).astype(a.dtype)
    s = np.sum([p.astype(np.int64) for p in parts], axis=0)
    return ((s + 2) >> 2).astype(a.dtype)


def parse_flags(flags):
    o = {"resolutions": "0", "halve": "mean", "height": -1, "width": -1, "depth": -1, "isotropic": False,
         "fixed_tiling": False, "V0": -1, "V1": -1, "H0": -1, "H1": -1, "D0": -1, "D1": -1}
    for f in flags:
        k, _, v = f.lstrip("-").partition("=")
        if k in ("isotropic", "fixed_tiling"):
            o[k] = True
        elif k in o and k not in ("resolutions", "halve"):
            o[k] = int(v)
        elif k in o:
            o[k] = v
    return o


def _tiles(total, block, fixed):
    n = int(math.ceil(total / np.float32(block)))
    if fixed:
        return [block if k < n - 1 else (block if total % block == 0 else total % block) for k in range(n)]
    return [total // n + (1 if k < total % n else 0) for k in range(n)]


def convert(vol, flags):
    """{relative .tif name: pages (N, h, w)} and {RES dir: mdata.bin bytes} of the conversion of series ``vol`` (D, V, H)."""
    o = parse_flags(flags)
    D, V, H = vol.shape
    V0 = max(o["V0"], 0)
    V1 = V if o["V1"] < 0 or o["V1"] > V else o["V1"]
    H0 = max(o["H0"], 0)
    H1 = H if o["H1"] < 0 or o["H1"] > H else o["H1"]
    D0 = max(o["D0"], 0)
    D1 = D if o["D1"] < 0 or o["D1"] > D else o["D1"]
    vol = vol[D0:D1, V0:V1, H0:H1]
    depth, height, width = vol.shape
    bh = height if o["height"] < 0 else o["height"]
    bw = width if o["width"] < 0 else o["width"]
    bd = depth if o["depth"] < 0 else o["depth"]
    assert bh >= 250 and bw >= 250
    sel = [str(i) in o["resolutions"] for i in range(10)]
    nres = max(i + 1 for i in range(10) if sel[i])
    hp = [0] * nres
    if o["isotropic"]:
        vx2, hx2, vd = np.float32(2), np.float32(2), np.float32(1)    # a 2-D series has unit voxels
        for i in range(1, nres):
            hp[i] = hp[i - 1]
            if vd <= max(vx2, hx2):
                hp[i] += 1
                vd *= 2
            vx2 *= 2
            hx2 *= 2
    else:
        hp = list(range(nres))
    rows = [_tiles(height // 2 ** i, bh, o["fixed_tiling"]) for i in range(nres)]
    cols = [_tiles(width // 2 ** i, bw, o["fixed_tiling"]) for i in range(nres)]
    # fixed tiling sizes the last D block from depth / 2^i whatever halve_pow2 says (VolumeConverter.cpp:1930)
    deps = []
    for i in range(nres):
        n = int(math.ceil((depth // 2 ** hp[i]) / np.float32(bd)))
        if o["fixed_tiling"]:
            last = depth // 2 ** i
            deps.append([bd if k < n - 1 else (bd if last % bd == 0 else last % bd) for k in range(n)])
        else:
            t = depth // 2 ** hp[i]
            deps.append([t // n + (1 if k < t % n else 0) for k in range(n)])
    zmr = max(min(64, bd // 2), 2 ** hp[nres - 1])
    if zmr > 1 and zmr > bd // 2:
        raise ValueError(f"too much resolutions({nres}): too much slices ({zmr}) in the buffer")
    vname = lambda i, r: str((V0 + r * 2 ** i) * 10).rjust(6, "0")
    hname = lambda i, c: str((H0 + c * 2 ** i) * 10).rjust(6, "0")
    dname = lambda i, s: str(D0 * 10 + 2 ** hp[i] * s * 10).rjust(6, "0")
    files, npages_tag = {}, {}
    blk = [0] * nres
    s_start = [0] * nres
    s_end = [deps[i][0] - 1 for i in range(nres)]
    z_ratio = depth // zmr
    for gi, z in enumerate(range(0, depth, zmr)):
        z_size = zmr if gi + 1 <= z_ratio else depth % zmr
        buf = vol[z:z + zmr]
        for i in range(nres):
            if z // 2 ** hp[i] > s_end[i]:
                # past the last block only in a leftover group too short to give a slice at this level (the reference then
                # reads past its table; nothing is written)
                blk[i] += 1
                s_start[i] = s_end[i] + 1
                s_end[i] += deps[i][blk[i]] if blk[i] < len(deps[i]) else 0
            if i:
                buf = halve3d(buf, o["halve"]) if hp[i] == hp[i - 1] + 1 else halve2d(buf, o["halve"])
            n = z_size // 2 ** hp[i]
            if not sel[i] or n <= 0:
                continue
            res = f"RES({height // 2 ** i}x{width // 2 ** i}x{depth // 2 ** hp[i]})"
            r0 = 0
            for r, nr in enumerate(rows[i]):
                c0 = 0
                for c, nc in enumerate(cols[i]):
                    vn, hn = vname(i, r0), hname(i, c0)
                    name, tag = f"{res}/{vn}/{vn}_{hn}/{vn}_{hn}_{dname(i, s_start[i])}.tif", deps[i][blk[i]]
                    changed = False
                    for bz in range(n):
                        if z // 2 ** hp[i] + bz > s_end[i] and not changed:
                            name, tag = f"{res}/{vn}/{vn}_{hn}/{vn}_{hn}_{dname(i, s_end[i] + 1)}.tif", deps[i][blk[i] + 1]
                            changed = True
                        files.setdefault(name, []).append(buf[bz, r0:r0 + nr, c0:c0 + nc])
                        npages_tag.setdefault(name, tag)
                    c0 += nc
                r0 += nr
    out = {k: np.stack(v) for k, v in files.items()}
    mdata = {}
    for i in range(nres):
        if not sel[i]:
            continue
        res = f"RES({height // 2 ** i}x{width // 2 ** i}x{depth // 2 ** hp[i]})"
        mdata[res] = _mdata(res, out, npages_tag, 2 ** i, 2 ** hp[i], vol.dtype.itemsize)
    return out, mdata


def _mdata(res, files, npages_tag, sv, sd, nbytes):
    """TiledVolume::save of the RES directory: blocks found by listing the tree, depths from the PAGENUMBER tags."""
    names = sorted(k[len(res) + 1:] for k in files if k.startswith(res + "/"))
    tree = {}
    for n in names:
        vdir, hdir, f = n.split("/")
        tree.setdefault(vdir, {}).setdefault(hdir, []).append(f)
    vdirs = sorted(tree)
    first = tree[vdirs[0]][sorted(tree[vdirs[0]])[0]][0][:-4].split("_")
    org = [np.float32(np.float32(int(v)) / np.float32(10000.0)) for v in first]
    blocks, dim_v, dim_h, dim_d = [], 0, 0, 0
    abs_v = 0
    for r, vd in enumerate(vdirs):
        abs_h = 0
        hdirs = sorted(tree[vd])
        for c, hd in enumerate(hdirs):
            fs = tree[vd][hd]
            shp = files[f"{res}/{vd}/{hd}/{fs[0]}"].shape
            sizes = [npages_tag[f"{res}/{vd}/{hd}/{f}"] for f in fs]
            blocks.append((shp[1], shp[2], sum(sizes), fs, sizes, abs_v, abs_h, f"{vd}/{hd}"))
            if r == 0:
                dim_h += shp[2]
            if c == 0:
                dim_v += shp[1]
            dim_d = max(dim_d, sum(sizes))
            abs_h += shp[2]
        abs_v += blocks[-1][0]
    b = struct.pack("<f3i", 2.0, 1, 2, 3)
    b += struct.pack("<6f", sv, sv, sd, sv, sv, sd) + struct.pack("<3f", *org)
    b += struct.pack("<3I2H", dim_v, dim_h, dim_d, len(vdirs), len(hdirs))
    for h, w, d, fs, sizes, av, ah, dirname in blocks:
        b += struct.pack("<5I2i", h, w, d, len(fs), 1, av, ah)
        b += struct.pack("<H", len(dirname) + 1) + dirname.encode() + b"\0"
        absd = 0
        for f, s in zip(fs, sizes):
            b += struct.pack("<H", len(f) + 1) + f.encode() + b"\0" + struct.pack("<Ii", s, absd)
            absd += s
        b += struct.pack("<I", nbytes)
    return b
