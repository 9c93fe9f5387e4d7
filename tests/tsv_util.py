"""TEST INFRASTRUCTURE for the TSVVolume merge (tests/test_tsv_host.py, tests/test_gpu_tsv.py, tests/golden/make_tsv_golden.py).

* the cases: grids of tiles made from seeds (never stored), the project XML of each, and where its golden lies;
* ``merge_restatement``: the merge in plain numpy, written from the description of the stage.  The golden maker
  and a CPU test require it to equal the reference's ``TSVVolume.imread`` exactly; it is the live comparison where there is no
  golden (synthetic stacks handed to ``mi_tsv_merge`` directly);
* ``import_reference``: the reference's ``tsv.volume`` with stand-ins for what is not installed -- golden maker ONLY.
"""
from __future__ import annotations

import sys
import types
from pathlib import Path

import numpy as np

GOLDEN_DIR = Path(__file__).resolve().parent / "golden" / "tsv"
PLACEHOLDER = "TILES_DIR"


# ---------------------------------------------------------------------------------------------------------------------------------
# cases

class Case:
    """One project: ``rows`` x ``cols`` tiles of ``height`` x ``width`` x ``slices`` samples; displacement triples (H, V, D) per stack."""

    def __init__(self, name, dtype, rows, cols, height, width, slices, overlap, seed, jitter=2, max_d=0, zero_h=False, blends=("max", "cosine"),
                 ignore_z_offsets=False, z_ranges=None):
        self.name, self.dtype, self.rows, self.cols = name, np.dtype(dtype), rows, cols
        self.height, self.width, self.slices, self.overlap, self.seed = height, width, slices, overlap, seed
        self.blends, self.ignore_z_offsets = blends, ignore_z_offsets
        self.z_ranges = z_ranges or {}      # (row, col) -> Z_RANGES attribute
        rng = np.random.default_rng(seed)
        self.north, self.west = {}, {}
        for r in range(rows):
            for c in range(cols):
                j = rng.integers(-jitter, jitter + 1, size=4) if jitter else np.zeros(4, int)
                d = rng.integers(0, max_d + 1, size=2)
                # a displacement is the negative of the step to the neighbour (make_stacks subtracts it)
                self.north[r, c] = (0 if zero_h else -int(j[0]), -(height - overlap + int(j[1])), int(d[0]))
                self.west[r, c] = (-(width - overlap + int(j[2])), -int(j[3]), int(d[1]))

    def dir_name(self, r, c):
        return f"{r * 1000:06}/{r * 1000:06}_{c * 1000:06}"

    def tile(self, r, c):
        """the samples of stack (r, c): [slices, height, width]; uint16 stays below 65520 (finite in float16)"""
        rng = np.random.default_rng([self.seed, r, c])
        top = 256 if self.dtype == np.uint8 else (65520, 4096, 300)[(r + 2 * c) % 3]
        return rng.integers(0, top, size=(self.slices, self.height, self.width)).astype(self.dtype)

    def xml(self, stacks_dir=PLACEHOLDER):
        """The project as TeraStitcher writes it after step 4, with what the merge must NOT read set to nonsense: ABS_* and a second
        entry in every displacement list."""
        def displ(tag, hvd):
            body = "".join(
                f'<Displacement TYPE="MIP_NCC"><V displ="{v}" default_displ="0" reliability="1" nccPeak="1" nccWidth="5" nccWRangeThr="10" '
                f'nccInvWidth="26" delay="0"/><H displ="{h}" default_displ="0" reliability="1" nccPeak="1" nccWidth="5" nccWRangeThr="10" '
                f'nccInvWidth="26" delay="0"/><D displ="{d}" default_displ="0" reliability="1" nccPeak="1" nccWidth="5" nccWRangeThr="10" '
                f'nccInvWidth="26" delay="0"/></Displacement>' for h, v, d in hvd)
            return f"<{tag}>{body}</{tag}>"

        stacks = []
        for r in range(self.rows):
            for c in range(self.cols):
                north = displ("NORTH_displacements", [self.north[r, c], (7, 7, 7)]) if r > 0 else "<NORTH_displacements/>"
                west = displ("WEST_displacements", [self.west[r, c], (-9, 9, 9)]) if c > 0 else "<WEST_displacements/>"
                z_ranges = self.z_ranges.get((r, c), f"[0,{self.slices})")
                stacks.append(
                    f'<Stack N_CHANS="1" N_BYTESxCHAN="{self.dtype.itemsize}" ROW="{r}" COL="{c}" ABS_V="{977 * r + 13}" ABS_H="{5 * c}" '
                    f'ABS_D="{3 * r}" STITCHABLE="yes" DIR_NAME="{self.dir_name(r, c)}" Z_RANGES="{z_ranges}" IMG_REGEX="">'
                    f"{north}<EAST_displacements/><SOUTH_displacements/>{west}</Stack>")
        return ('<?xml version="1.0" encoding="UTF-8" ?>\n<!DOCTYPE TeraStitcher SYSTEM "TeraStitcher.DTD">\n'
                '<TeraStitcher volume_format="TiledXY|2Dseries" input_plugin="tiff2D">'
                f'<stacks_dir value="{stacks_dir}"/><ref_sys ref1="1" ref2="2" ref3="3"/><voxel_dims V="2" H="2" D="5"/>'
                f'<origin V="0" H="0" D="0"/><mechanical_displacements V="{2 * (self.height - self.overlap)}" H="{2 * (self.width - self.overlap)}"/>'
                f'<dimensions stack_rows="{self.rows}" stack_columns="{self.cols}" stack_slices="{self.slices}"/>'
                f'<STACKS>{"".join(stacks)}</STACKS></TeraStitcher>\n')

    def kept_indices(self, r, c):
        """the slice indices Z_RANGES keeps of stack (r, c)"""
        z = self.z_ranges.get((r, c))
        if z is None:
            return list(range(self.slices))
        out = []
        for part in z.split(";"):
            a, b = (int(v) for v in part[1:-1].split(","))
            out += list(range(a, b))
        return out

    def golden_path(self):
        return GOLDEN_DIR / f"{self.name}.npz"

    def stored_xml(self):
        """the XML beside the golden (stacks_dir = the placeholder): what the reference read when the golden was made"""
        return (GOLDEN_DIR / f"{self.name}.xml").read_text()

    def write(self, folder, imsave, xml_text=None):
        """tiles as ``<folder>/tiles/<DIR_NAME>/t<50 * z>.tif`` through ``imsave(path, plane)`` and the XML (``xml_text`` with the placeholder
        replaced, or the case's own); returns the XML path.
        The names sort as strings in another order (t0, t100, t150, t200, t50) than by their integers."""
        folder = Path(folder)
        tiles = folder / "tiles"
        for r in range(self.rows):
            for c in range(self.cols):
                d = tiles / self.dir_name(r, c)
                d.mkdir(parents=True, exist_ok=True)
                for z, plane in enumerate(self.tile(r, c)):
                    imsave(d / f"t{z * 50}.tif", plane)
        xml = folder / f"{self.name}.xml"
        xml.write_text(self.xml(str(tiles)) if xml_text is None else xml_text.replace(PLACEHOLDER, str(tiles)))
        return xml


_A = dict(dtype=np.uint16, height=40, width=56, slices=5, overlap=12)
CASES = {c.name: c for c in (
    Case("A", rows=2, cols=3, seed=11, max_d=2, **_A),
    Case("B", np.uint16, 3, 3, 64, 64, 2, 20, seed=12),
    Case("C", np.uint8, 2, 2, 47, 81, 3, 16, seed=13),
    Case("D", rows=3, cols=1, seed=14, max_d=2, zero_h=True, **_A),
    Case("E", np.uint16, 1, 2, 300, 300, 1, 260, seed=15, blends=("cosine",)),
    Case("F_ignore_z", rows=2, cols=3, seed=11, max_d=2, ignore_z_offsets=True, **_A),
    Case("F_z_ranges", rows=2, cols=3, seed=11, max_d=2, z_ranges={(0, 1): "[0,3);[4,5)"}, **_A),
)}
EXACT_CASES = ("A", "B", "C", "D", "F_ignore_z", "F_z_ranges")


def load_golden(case):
    """dict: x0 / y0 / z0 [rows, cols], extent [6] = x0 x1 y0 y1 z0 z1, and ``max`` / ``cosine`` volumes [z, y, x]"""
    with np.load(case.golden_path()) as f:
        return {k: f[k] for k in f.files}


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement

def place_restatement(case):
    """offsets x0 / y0 / z0 [rows, cols] and the extent, from the case's displacement triples"""
    R, Cc = case.rows, case.cols
    off = np.zeros((R, Cc, 3), np.int64)   # x, y, z
    for r in range(R):
        for c in range(Cc):
            if r == 0 and c == 0:
                continue
            prev, (h, v, d) = (off[r - 1, c], case.north[r, c]) if r > 0 else (off[r, c - 1], case.west[r, c])
            off[r, c] = prev - np.array([h, v, 0 if case.ignore_z_offsets else d])
    off -= off.reshape(-1, 3).min(axis=0)
    nz = np.array([[len(case.kept_indices(r, c)) for c in range(Cc)] for r in range(R)])
    extent = (off[..., 0].min(), off[..., 0].max() + case.width, off[..., 1].min(), off[..., 1].max() + case.height,
              off[..., 2].min(), (off[..., 2] + nz).max())
    return off[..., 0], off[..., 1], off[..., 2], tuple(int(v) for v in extent)


def _edge_distance(sx, sy, ox, oy, H, W, X, Y):
    """[len(Y), len(X)]: the distance of stack s = (sx, sy) from its edges inside its overlap with o, at absolute X / Y.  float32 until
    a ramp of int64 positions is taken into the minimum, float64 from then on (numpy's promotion, as in the reference): with any edge
    flagged the weight is computed in float64."""
    ax0, ax1, ay0, ay1 = max(sx, ox), min(sx, ox) + W, max(sy, oy), min(sy, oy) + H
    most = np.inf
    if sx != ox:
        most = ax1 - ax0
    if sy != oy:
        most = min(most, ay1 - ay0)
    assert np.isfinite(most), "two stacks on one XY rectangle"
    d = np.full((len(Y), len(X)), most, np.float32)
    if ox < sx < ox + W:
        d = np.minimum(d, (X - ax0 + 1)[None, :])
    if ox < sx + W < ox + W:
        d = np.minimum(d, (ax1 - X)[None, :])
    if oy < sy < oy + H:
        d = np.minimum(d, (Y - ay0 + 1)[:, None])
    if oy < sy + H < oy + H:
        d = np.minimum(d, (ay1 - Y)[:, None])
    return d


def merge_restatement(stacks, x0, y0, z0, box, cosine):
    """The box (bx0, bx1, by0, by1, bz0, bz1) of the volume of ``stacks`` (list of [nz, H, W] arrays in blend order) at x0 / y0 / z0."""
    dtype = stacks[0].dtype
    H, W = stacks[0].shape[1:]
    bx0, bx1, by0, by1, bz0, bz1 = (int(v) for v in box)
    shape = (bz1 - bz0, by1 - by0, bx1 - bx0)

    def clipped(s):
        e = (max(int(x0[s]), bx0), min(int(x0[s]) + W, bx1), max(int(y0[s]), by0), min(int(y0[s]) + H, by1),
             max(int(z0[s]), bz0), min(int(z0[s]) + stacks[s].shape[0], bz1))
        return e if e[0] < e[1] and e[2] < e[3] and e[4] < e[5] else None

    def rel(e, ox, oy, oz):
        return slice(e[4] - oz, e[5] - oz), slice(e[2] - oy, e[3] - oy), slice(e[0] - ox, e[1] - ox)

    parts = [(s, clipped(s)) for s in range(len(stacks))]
    parts = [(s, e) for s, e in parts if e is not None]
    if not cosine:
        out = np.zeros(shape, dtype)
        for s, e in parts:
            view = out[rel(e, bx0, by0, bz0)]
            np.maximum(view, stacks[s][rel(e, int(x0[s]), int(y0[s]), int(z0[s]))], out=view)
        return out
    f16 = np.float16
    result, multiplier = np.zeros(shape, f16), np.zeros(shape, f16)
    for s, e in parts:
        with np.errstate(over="ignore"):   # a uint16 sample from 65520 on is inf in float16
            part = stacks[s][rel(e, int(x0[s]), int(y0[s]), int(z0[s]))].astype(f16)
        mpart = np.ones(part.shape, f16)
        for o, eo in parts:
            if o == s:
                continue
            k = (max(e[0], eo[0]), min(e[1], eo[1]), max(e[2], eo[2]), min(e[3], eo[3]), max(e[4], eo[4]), min(e[5], eo[5]))
            if not (k[0] < k[1] and k[2] < k[3] and k[4] < k[5]):
                continue
            X, Y = np.arange(k[0], k[1]), np.arange(k[2], k[3])
            d = _edge_distance(int(x0[s]), int(y0[s]), int(x0[o]), int(y0[o]), H, W, X, Y)
            od = _edge_distance(int(x0[o]), int(y0[o]), int(x0[s]), int(y0[s]), H, W, X, Y)
            w = (np.sin(np.arctan2(d, od)) ** 2).astype(f16)[None]
            sub = rel(k, e[0], e[2], e[4])
            part[sub] *= w
            mpart[sub] *= w
        result[rel(e, bx0, by0, bz0)] += part
        multiplier[rel(e, bx0, by0, bz0)] += mpart
    eps = np.finfo(f16).eps
    with np.errstate(all="ignore"):
        result = np.where(multiplier > eps, result / multiplier, result / eps)
    top = np.float32(np.iinfo(dtype).max)
    r32 = result.astype(np.float32)
    # inf / nan saturate (the departure); for uint8 this is also the reference's clip; the cast truncates
    return np.where(np.isfinite(r32) & (r32 < top), r32, top).astype(dtype)


def sub_boxes(extent):
    """Boxes whose result must be the same slice of the full read: an odd x0 (and odd width); a single z; a box wholly outside every
    stack; two boxes that straddle the covered / uncovered edge (past the far corner, and before the origin)."""
    x0, x1, y0, y1, z0, z1 = extent
    zm = z0 + (z1 - z0) // 2
    return [(x0 + 7 + (x0 % 2 == 0) - 1 + 1, x1 - 4, y0 + 3, y1 - 2, z0, z1),
            (x0, x1, y0, y1, zm, zm + 1),
            (x1 + 3, x1 + 20, y0 + 1, y0 + 9, z0, z0 + 1),
            (x1 - 9, x1 + 6, y1 - 7, y1 + 4, z0, z1),
            (x0 - 5, x0 + 11, y0 - 3, y0 + 8, z1 - 1, z1 + 2)]


def slice_of(full, extent, box):
    """the box of the volume whose full read (of ``extent``) is ``full``; zeros outside the extent"""
    out = np.zeros((box[5] - box[4], box[3] - box[2], box[1] - box[0]), full.dtype)
    lo = [max(box[2 * i], extent[2 * i]) for i in range(3)]       # x, y, z
    hi = [min(box[2 * i + 1], extent[2 * i + 1]) for i in range(3)]
    if all(a < b for a, b in zip(lo, hi)):
        out[lo[2] - box[4]:hi[2] - box[4], lo[1] - box[2]:hi[1] - box[2], lo[0] - box[0]:hi[0] - box[0]] = \
            full[lo[2] - extent[4]:hi[2] - extent[4], lo[1] - extent[2]:hi[1] - extent[2], lo[0] - extent[0]:hi[0] - extent[0]]
    return out


def case_stacks(case):
    """(stacks in blend order with Z_RANGES applied, x0, y0, z0 flattened, extent) of a case"""
    x0, y0, z0, extent = place_restatement(case)
    stacks = [case.tile(r, c)[case.kept_indices(r, c)] for r in range(case.rows) for c in range(case.cols)]
    return stacks, x0.reshape(-1), y0.reshape(-1), z0.reshape(-1), extent


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference (golden maker only)

def import_reference(reference_root, imread):
    """The reference's ``tsv.volume`` on this machine: the stand-ins of tests/pystripe_util.py for what ``pystripe.core`` imports,
    ``tifffile.imread`` = ``imread``, and its numpy branch (USE_NUMEXPR = False; numexpr is not installed)."""
    from tests.pystripe_util import install_standins
    install_standins()
    sys.modules["tifffile"].imread = imread
    if "psutil" not in sys.modules:
        try:
            import psutil  # noqa: F401
        except ImportError:
            sys.modules["psutil"] = types.ModuleType("psutil")
    if reference_root not in sys.path:
        sys.path.insert(0, reference_root)
    import tsv.volume as tv
    tv.USE_NUMEXPR = False
    tv.imread = imread
    return tv
