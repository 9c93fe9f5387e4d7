"""CPU: the host side of channel alignment (include/mi_align.h, ipp_amd.align_images, mi_tiff_write_rgb_series) and the restatement
of tests/channel_align_util.py itself: its sobel, blur and gradients against scipy.ndimage, its factored sums against the two-pass
form, its ECC against a synthetic truth; then, with no tolerance, the array plumbing, the composite index map, alignments.txt,
the scaled offsets, the parser, every refusal and the RGB writer."""
import os
from argparse import Namespace

import numpy as np
import pytest
import scipy.ndimage as ndi

from tests import channel_align_util as U
from tests.conftest import ROOT

GOLDEN = os.path.join(ROOT, "tests", "golden", "channel_align", "recorded.npz")
SHAPES = list(U.ECC_CASES)
TRANSLATIONS = [(0.0, 0.0), (0.5, -0.25), (2.3, -1.7), (-6.0, 4.0)]


@pytest.fixture(scope="module")
def ai():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import align_images
    return align_images


@pytest.fixture(scope="module")
def recorded():
    return np.load(GOLDEN)


def plane(shape, seed=1):
    return (np.random.default_rng(seed).random(shape) * 4000).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------------------
# the restatement against scipy.ndimage

@pytest.mark.parametrize("shape", SHAPES + [(1, 7), (2, 2)])
def test_restatement_sobel_is_scipy_convolution_with_the_two_kernels(shape):
    """scipy accumulates in float64 too, in its own order: after the rounding to float32 the two h (and v) differ by at most one
    float32 spacing, so the magnitude by a few 2^-24 of itself plus the same share of the largest sample"""
    img = plane(shape)
    edge, smooth = np.array([1.0, 0.0, -1.0]), np.array([1.0, 2.0, 1.0])
    kh, kv = np.outer(edge, smooth) / 8.0, np.outer(smooth, edge) / 8.0
    h = ndi.convolve(img, kh, output=np.float32, mode="reflect")
    v = ndi.convolve(img, kv, output=np.float32, mode="reflect")
    want = np.sqrt((h * h + v * v) / np.float32(2))
    got = U.sobel(img)
    assert got.dtype == np.float32
    assert np.all(np.abs(got - want) <= 4 * 2.0 ** -24 * (np.abs(want) + np.abs(img).max()))


@pytest.mark.parametrize("shape", SHAPES + [(3, 3)])
def test_restatement_blur_and_gradients_are_correlate1d_mirror(shape):
    """the same taps through scipy (float64 inside): the float32 restatement stays within 5 float32 roundings per pass"""
    img = plane(shape, 2)
    taps = np.array([1, 4, 6, 4, 1]) / 16.0
    want = ndi.correlate1d(ndi.correlate1d(img.astype(np.float64), taps, axis=1, mode="mirror"), taps, axis=0, mode="mirror")
    got = U.blur5(img)
    assert got.dtype == np.float32
    assert np.all(np.abs(got - want) <= 12 * 2.0 ** -24 * np.abs(img).max())
    gx, gy = U.gradients(got)
    d = np.array([-0.5, 0.0, 0.5])
    # 0.5 * a - 0.5 * b in float32 is the rounded exact difference: equal to scipy's float64 result rounded once
    assert np.array_equal(gx, ndi.correlate1d(got.astype(np.float64), d, axis=1, mode="mirror").astype(np.float32))
    assert np.array_equal(gy, ndi.correlate1d(got.astype(np.float64), d, axis=0, mode="mirror").astype(np.float32))


def test_warp_at_integer_translations_is_a_shift_with_zeros():
    a = plane((9, 11), 3)
    w = U.warp(a, -6.0, 4.0)
    assert np.array_equal(w[:5, 6:], a[4:, :5]) and not w[5:].any() and not w[:, :6].any()
    assert np.array_equal(U.mask(a.shape, -6.0, 4.0), w != 0)
    assert np.array_equal(U.warp(a, 0.0, 0.0), a)


@pytest.mark.parametrize("shape", SHAPES)
def test_factored_sums_match_the_two_pass_form(shape, recorded):
    """A factored quantity is a difference a - b of sums that each carry a few float64 roundings of their own size; against the
    natural scale of the result (util.natural_scale) that is a few 2^-53 times the cancellation factor kappa = (raw second moment) /
    (centred second moment) of the two images.  The largest value met is recorded in the golden file and quoted in DESIGN."""
    tmpl, subj, _ = U.ecc_case(shape)
    planes = U.ecc_prepare(tmpl, subj)
    for t in TRANSLATIONS:
        sums, _ = U.ecc_sums(planes, *t)
        if sums[0] == 0:
            continue
        S = dict(zip(U.SUM_NAMES, sums))
        one, two = U.derived(sums), U.derived_two_pass(planes, *t)
        kappa = max(S["sww"] / two["wn2"], S["stt"] / two["tn2"], 1.0)
        for k, v in two.items():
            scale = U.natural_scale(k, two)
            rel = abs(one[k] - v) / scale
            print(shape, t, k, rel)
            assert rel <= 16 * 2.0 ** -53 * kappa, (shape, t, k, rel, kappa)
            assert rel <= float(recorded["factoring_rel"]) * (1 + 1e-6)


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_ecc_recovers_a_known_subpixel_shift(k, recorded):
    shape = tuple(int(v) for v in recorded["ecc_shapes"][k])
    tmpl, subj, truth = U.ecc_case(shape)
    tx, ty, rho, count, status = U.ecc_translation(tmpl, subj)
    assert status == U.ECC_OK and rho > 0.97
    assert truth == tuple(recorded["ecc_truth"][k])
    error = max(abs(tx - truth[0]), abs(ty - truth[1]))
    print(shape, tx, ty, count, error)
    assert abs(error - recorded["ecc_error"][k]) < 1e-6 and count == recorded["ecc_iterations"][k]
    # the borders limit what a plane this small can tell: a fifth of a pixel on 9 x 11, a twentieth from 37 x 53 on
    assert error < (0.2 if min(shape) < 16 else 0.05)


def test_ecc_failure_statuses_of_the_restatement():
    flat = np.full((20, 24), 7.0, np.float32)
    assert U.ecc_translation(flat, flat)[4] == U.ECC_NAN                       # no gradient, no variance
    a = U.smooth_plane((20, 24), 3)()
    planes = U.ecc_prepare(a, a)
    assert U.ecc_step(U.ecc_sums(planes, 40.0, 0.0)[0])[3] == U.ECC_NAN          # the shift empties the mask
    assert U.ecc_translation(a, (300 - a).astype(np.float32))[4] == U.ECC_MINIMIZED   # anticorrelated


def test_recorded_outer_loops_keep_their_margin(recorded):
    assert recorded["align_margin"] >= 0.1 and recorded["main_margin"] >= 0.1
    assert U.half_integer_margin(recorded["align_sums"]) == recorded["align_margin"]
    assert recorded["align_moves"].sum(axis=1).tolist() == [-3, 2, -1]


# ---------------------------------------------------------------------------------------------------------------------------------
# array plumbing: equal, on numpy arrays and on torch tensors

def _both(a):
    import torch
    t = torch.from_numpy(a.copy())
    return [("numpy", a.copy(), lambda x: x), ("torch", t, lambda x: x.view(torch.int16).numpy().view(np.uint16) if x.dtype == torch.uint16 else x.numpy())]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_roll_pad_pad_and_trim(ai, dtype):
    vol = (np.random.default_rng(4).integers(1, 250, (5, 6, 7))).astype(dtype)
    for name, arr, host in _both(vol):
        for axis in (0, 1, 2):
            for move in (0, 1, -2, 4, -4, vol.shape[axis], -vol.shape[axis] - 3):
                got = arr.copy() if name == "numpy" else arr.clone()
                want = vol.copy()
                ai.roll_pad(got, move, axis=axis)
                U.roll_pad(want, move, axis=axis)
                assert np.array_equal(host(got), want), (name, axis, move)
        for shape in ((5, 6, 7), (6, 9, 8), (10, 6, 12)):
            padded = ai.pad_to_shape(shape, arr)
            assert np.array_equal(host(padded), U.pad_to_shape(shape, vol)), (name, shape)
            assert np.array_equal(host(ai.trim_to_shape(vol.shape, padded)), vol)
        for shape in ((5, 6, 7), (2, 3, 4), (4, 6, 1)):
            assert np.array_equal(host(ai.trim_to_shape(shape, arr)), U.trim_to_shape(shape, vol)), (name, shape)
        with pytest.raises(Exception):
            ai.roll_pad(arr, 1, axis=3)
    assert ai.trim_to_shape((1, 1), None) is None


def test_resize_arrays_and_get_layer(ai):
    a, b = np.ones((3, 4, 5), np.uint16), np.full((4, 4, 2), 2, np.uint16)
    out = ai.resize_arrays([a.copy(), None, b.copy()])
    assert out[1] is None and out[0].shape == out[2].shape == (4, 4, 5)
    assert np.array_equal(out[0], U.pad_to_shape((4, 4, 5), a)) and np.array_equal(out[2], U.pad_to_shape((4, 4, 5), b))
    vol = np.arange(2 * 3 * 4).reshape(2, 3, 4)
    for plane_name in ("xy", "xz", "yz"):
        assert np.array_equal(ai.get_layer(1, vol, plane_name), U.get_layer(1, vol, plane_name))
    assert np.array_equal(ai.get_layer(1, vol, "yx"), vol[1]) and ai.get_layer(0, vol, "ab") is None and ai.get_layer(0, None) is None


def _apply_map(volumes, maps, out_shape, out_dtype):
    """the index map applied with plain numpy indexing (what the kernel does)"""
    n, ny, nx = out_shape
    out = np.zeros((n, ny, nx, 3), out_dtype)
    for c, (v, m) in enumerate(zip(volumes, maps)):
        if v is None:
            continue
        for k in range(n):
            for y in range(ny):
                zs, ys = k + m[0], y + m[1]
                if not (0 <= zs < v.shape[0] and 0 <= ys < v.shape[1]):
                    continue
                x0, x1 = max(0, -m[2]), min(nx, v.shape[2] - m[2])
                if x0 < x1:
                    out[k, y, x0:x1, c] = v[zs, ys, x0 + m[2]:x1 + m[2]].astype(out_dtype)
    return out


COMPOSITE_CASES, composite_volumes = U.COMPOSITE_CASES, U.composite_volumes


@pytest.mark.parametrize("case", list(COMPOSITE_CASES))
def test_composite_index_map_is_the_four_numpy_steps(ai, case):
    shapes, reference, offsets = COMPOSITE_CASES[case]
    for src, out in ((np.uint8, np.uint8), (np.uint16, np.uint8), (np.uint16, np.uint32), (np.uint8, np.float32), (np.uint16, np.uint16)):
        volumes = composite_volumes(shapes, src)
        maps = ai.composite_index_map(shapes, reference, offsets)
        assert [m is None for m in maps] == [s is None for s in shapes]
        want = U.composite(volumes, reference, offsets, out)
        got = _apply_map(volumes, maps, shapes[reference], out)
        assert want.dtype == got.dtype and np.array_equal(got, want), case
        if case == "larger-than-the-extent":
            assert not want[..., 1].any() and not want[..., 2].any() and want[..., 0].any()


def test_alignments_txt_text_and_fallback_name(ai, tmp_path):
    channels = [[None, None, None], [-3, 2, 0], [1, -2, -1]]
    files = ["/data/r down", "/data/g", None]
    residuals = [None, (np.float32(0.25), np.float32(-0.125), np.float32(0.5)), None]
    for n, name in enumerate(["alignments.txt", "alignments (1).txt", "alignments (2).txt"]):
        path = ai.write_alignments(channels, files, residuals, n % 2, tmp_path)
        assert path == tmp_path / name
        assert open(path).read() == U.alignments_text(channels, files, residuals, n % 2)
    text = open(tmp_path / "alignments.txt").read()
    assert text.startswith("Number of channels: 3\n\t Channel 0: /data/r down\n\t Channel 1: /data/g\n\t Channel 2: None\nReference channel: 0\n"
                           # kept: the headings count on past the reference while the entries start at the list's first
                           "Channel 1:\n\tx-alignment: None\n\ty-alignment: None\n\tz-alignment: None\n\n"
                           "Channel 2:\n\tx-alignment: -3\t\t Residuals: 0.25\n")
    assert text.endswith("Channel 3:\n\tx-alignment: 1\n\ty-alignment: -2\n\tz-alignment: -1\n\n")


def test_scaled_offsets_take_the_moves_in_z_y_x_order(ai):
    alignments = [[None, None, None], [-3, 2, 5], [7, -9, -1]]
    got = ai.scaled_alignments(alignments, 0, (1, 2), (1, 4), (3, 2))
    assert got == [[0, 0, 0], [int(5 / 1.5), int(2 / 0.25), int(-3 / 0.5)], [int(-1 / 1.5), int(-9 / 0.25), int(7 / 0.5)]]
    assert got[1] == [3, 8, -6] and got[2] == [0, -36, 14]          # int() truncates toward zero
    assert ai.scaled_alignments(alignments, 2, (1, 1), (1, 1), (1, 1)) == [[0, 0, 0], [5, 2, -3], [0, 0, 0]]


def test_parser_wiring(ai):
    a = ai.build_parser().parse_args(["--red", "ro", "rd", "-g", "go", "gd", "--output", "out", "--dx", "1", "2", "--dy", "3", "4", "--dz", "5", "6"])
    assert (a.red, a.green, a.blue, a.output) == (["ro", "rd"], ["go", "gd"], [None, None], "out")
    assert (a.dx, a.dy, a.dz) == ([1, 2], [3, 4], [5, 6])
    assert (a.max_iterations, a.reference, a.num_threads, a.dtype) == (10, "red", 8, "uint8")
    assert not (a.write_alignments or a.generate_ims or a.save_singles)
    b = ai.build_parser().parse_args(["-b", "bo", "bd", "-r", "ro", "rd", "-o", "x", "--dx", "1", "1", "--dy", "1", "1", "--dz", "1", "1", "--reference", "Blue ",
                                      "--max_iterations", "3", "--write_alignments", "--dtype", "uint32", "--num_threads", "2"])
    assert (b.blue, b.reference, b.max_iterations, b.write_alignments, b.dtype, b.num_threads) == (["bo", "bd"], "Blue ", 3, True, "uint32", 2)
    assert [ai.reference_index(s) for s in ("red", "R", " Green", "g", "Blue ", "b")] == [0, 0, 1, 1, 2, 2]
    with pytest.raises(SystemExit):
        ai.reference_index("cyan")
    with pytest.raises(SystemExit):
        ai.build_parser().parse_args(["--red", "ro", "rd"])          # --output and the voxel sizes are required


def _args(**over):
    base = dict(red=("r", "rd"), green=("g", "gd"), blue=(None, None), output="o", max_iterations=10, write_alignments=False, reference="red",
                num_threads=2, generate_ims=False, save_singles=False, dtype="uint8", dx=(1, 2), dy=(1, 2), dz=(1, 2))
    base.update(over)
    return Namespace(**base)


def test_every_refusal_names_its_argument(ai, tmp_path):
    for over, word in ((dict(generate_ims=True), "generate_ims"), (dict(save_singles=True), "save_singles"), (dict(dtype="float64"), "float64")):
        with pytest.raises(NotImplementedError, match=word):
            ai.main(_args(**over))
    with pytest.raises(NotImplementedError, match="save_singles"):
        ai.write_to_file([], [], 0, tmp_path / "a", "uint8", save_singles=True)
    with pytest.raises(NotImplementedError, match="save_singles"):
        ai.process_big_images([], tmp_path / "b", 0, [], save_singles=True)
    with pytest.raises(NotImplementedError, match="float64"):
        ai.write_to_file([], [], 0, tmp_path / "c", "float64")
    with pytest.raises(NotImplementedError, match="mode"):
        ai.pad_to_shape((3, 3), np.zeros((2, 2)), mode="edge")
    with pytest.raises(SystemExit):
        ai.main(_args(green=(None, None)))                            # fewer than two channels
    with pytest.raises(SystemExit):
        ai.main(_args(red=(str(tmp_path / "missing"), str(tmp_path / "missing"))))


def test_downsampling_factor_and_block_reduce(ai):
    import torch
    assert ai.downsampling_factor((100, 32767), (100, 200)) == 1
    assert ai.downsampling_factor((100, 32768), (100, 200)) == 2
    assert ai.downsampling_factor((3, 70000), (140000, 5)) == 8
    a = np.random.default_rng(8).random((5, 11)).astype(np.float32) * 100
    got = ai._block_reduce_mean(torch.from_numpy(a), 4).numpy()
    want = U.block_reduce_mean(a, 4)
    # 16 float32 samples per block summed in float32: 16 roundings of the block's sum at most
    assert got.shape == want.shape == (2, 3) and np.all(np.abs(got - want) <= 16 * 2.0 ** -24 * 100)
    m = ai.get_transformation_matrix(None, None, verbose=False)
    assert m.dtype == np.float32 and np.array_equal(m, np.eye(3, dtype=np.float32))


# ---------------------------------------------------------------------------------------------------------------------------------
# the RGB writer

RGB_DTYPES = [np.uint8, np.uint16, np.uint32, np.float32]


def rgb_volume(dtype, shape=(3, 37, 53, 3)):
    rng = np.random.default_rng(9)
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal(shape) * 1000).astype(np.float32)
    smooth = np.cumsum(rng.integers(0, 3, shape), axis=2)             # compressible, and above 2^16 for uint32
    return (smooth * (70000 if np.dtype(dtype) == np.uint32 else 1)).astype(dtype)


@pytest.mark.parametrize("compression", [None, "deflate"])
@pytest.mark.parametrize("dtype", RGB_DTYPES)
def test_rgb_writer_round_trip(ai, tmp_path, dtype, compression):
    vol = rgb_volume(dtype)
    paths = [tmp_path / f"{k}.tif" for k in range(vol.shape[0])]
    assert ai.write_rgb_series(paths, vol, compression=compression, level=6) == vol.shape[0]
    assert not list(tmp_path.glob("*.tmp"))
    for k, p in enumerate(paths):
        arr, tags = U.read_tiff(p)
        assert arr.dtype == vol.dtype and np.array_equal(arr, vol[k])
        assert tags[277] == [3] and tags[262] == [2] and tags[284] == [1] and tags[259] == [8 if compression else 1]
        assert tags[258] == [8 * vol.dtype.itemsize] * 3 and tags[339] == [3 if dtype == np.float32 else 1] * 3
        if dtype == np.uint8:
            from PIL import Image
            with Image.open(p) as im:
                assert im.mode == "RGB" and np.array_equal(np.asarray(im), vol[k])
    if compression and dtype != np.float32:
        assert os.path.getsize(paths[0]) < vol[0].nbytes
    # multi-sample files stay outside the fast reader
    from ipp_amd import brickio
    assert brickio.tiff_info(paths[0])[2] is False


def test_rgb_writer_many_strips_and_existing_files(ai, tmp_path):
    vol = rgb_volume(np.uint16, (2, 700, 301, 3))                     # 1 806 bytes per row: 580 rows per strip, two strips
    paths = [tmp_path / "a.tif", tmp_path / "b.tif"]
    paths[0].write_bytes(b"kept")
    assert ai.write_rgb_series(paths, vol) == 1
    assert paths[0].read_bytes() == b"kept"
    arr, tags = U.read_tiff(paths[1])
    assert len(tags[273]) == 2 and tags[278] == [580] and np.array_equal(arr, vol[1])
    assert ai.write_rgb_series(paths, vol) == 0
    with pytest.raises(ValueError):
        ai.write_rgb_series(paths, vol[..., :2])
    with pytest.raises(ValueError):
        ai.write_rgb_series(paths, vol.astype(np.float64))
