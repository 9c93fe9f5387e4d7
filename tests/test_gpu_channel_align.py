"""GPU: channel alignment and the RGB composite (include/mi_align.h, ipp_amd.align_images) against the numpy restatement of
tests/channel_align_util.py.  Float32 arithmetic in a fixed order (blur, gradients, composite) is equal to the restatement; sobel and
the float64 sums are checked to the bound their accumulation gives; the ECC translation to 1e-3 pixel, a tenth of the 0.01 pixel the
reference's own ``transformation_is_needed`` resolves; the outer loop's integer moves and everything written to disk are equal."""
import functools
import hashlib
import os
from argparse import Namespace

import numpy as np
import pytest

from tests import channel_align_util as U
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

# under one wave and the smallest for the 5-tap mirror border; odd with a vector head and tail; rows of whole 16-byte groups;
# several work-groups and a multi-row partial buffer
SHAPES = [(9, 11), (37, 53), (64, 64), (131, 257)]
TRANSLATIONS = [(0.0, 0.0), (0.5, -0.25), (2.3, -1.7), (-6.0, 4.0)]


@pytest.fixture(scope="module")
def ai(dev):
    from ipp_amd import align_images
    return align_images


@pytest.fixture(scope="module")
def recorded():
    return np.load(os.path.join(ROOT, "tests", "golden", "channel_align", "recorded.npz"))


@functools.lru_cache(maxsize=None)
def case(shape):
    """(template, subject, truth, the restatement's prepared planes), read-only"""
    tmpl, subj, truth = U.ecc_case(shape)
    planes = U.ecc_prepare(tmpl, subj)
    for a in (tmpl, subj) + tuple(planes):
        a.setflags(write=False)
    return tmpl, subj, truth, planes


@functools.lru_cache(maxsize=None)
def restated_run(shape):
    tmpl, subj, _, _ = case(shape)
    return U.ecc_translation(tmpl, subj)


def to_dev(a, dev):
    import torch
    return torch.from_numpy(np.array(a)).to(dev)


@pytest.mark.parametrize("shape", SHAPES + [(1, 5), (2, 2)])
def test_sobel_within_the_bound_of_float64_accumulation(ai, dev, shape):
    """h and v are float64 sums of six exact products whose weights add up to 1: in any order they are off by at most
    5 * 2^-53 * max|a|.  Rounded to float32, two such values differ by at most one float32 spacing, 2^-23 |h|, so through
    out = sqrt((h^2 + v^2) / 2) by (|dh| |h| + |dv| |v|) / (2 out) <= 2^-23 out.  The float32 part (two squares, a sum, an exact
    halving, a correctly rounded root) adds at most 2.5 * 2^-24 out on either side.  Together: 7 * 2^-24 out; the test allows
    8 * 2^-24 out + 2^-40 max|a| (the second term covers the float64 part and the underflow of tiny squares)."""
    img = (np.random.default_rng(1).random(shape) * 4000).astype(np.float32)
    want = U.sobel(img)
    got = ai.get_gradient(to_dev(img, dev)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    bound = 8 * 2.0 ** -24 * want + 2.0 ** -40 * np.abs(img).max()
    print(shape, "largest error / bound", float((err / bound).max()), "unequal pixels", int((got != want).sum()))
    assert np.all(err <= bound)
    # the pipeline's planes are uint16 views taken from a volume: the same values through the integer path
    u16 = (img * 10).astype(np.uint16)
    assert np.array_equal(ai.get_gradient(to_dev(u16.T.copy(), dev).T).cpu().numpy(), ai.get_gradient(to_dev(u16.astype(np.float32), dev)).cpu().numpy())


@pytest.mark.parametrize("shape", SHAPES + [(3, 3)])
def test_blur_and_gradients_equal_the_restatement(ai, dev, shape):
    rng = np.random.default_rng(2)
    tmpl, subj = (rng.random(shape) * 4000).astype(np.float32), (rng.random(shape) * 300).astype(np.float32)
    got = [p.cpu().numpy() for p in ai.ecc_prepare(to_dev(tmpl, dev), to_dev(subj, dev))]
    for name, g, w in zip(("t", "s", "gx", "gy"), got, U.ecc_prepare(tmpl, subj)):
        assert g.dtype == np.float32 and np.array_equal(g, w), (shape, name, float(np.abs(g - w).max()))


@pytest.mark.parametrize("unaligned", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_ecc_sums_within_the_reordering_bound_and_bit_equal_twice(ai, dev, shape, unaligned):
    """Every term is a product of float32 values, exact in float64, so the device's sum and the restatement's differ only in the
    order of n additions: by at most n * 2^-53 * sum|term|, computed per sum from the fixture."""
    import torch
    _, _, _, planes = case(shape)
    n = shape[0] * shape[1]
    if unaligned:   # planes that start one element off a 16-byte boundary: the element-wise route for the template
        held = [torch.empty(n + 1, dtype=torch.float32, device=dev) for _ in planes]
        device_planes = [h[1:].view(shape).copy_(to_dev(p, dev)) for h, p in zip(held, planes)]
        assert all(p.data_ptr() % 16 == 4 for p in device_planes)
    else:
        device_planes = [to_dev(p, dev) for p in planes]
    for tx, ty in TRANSLATIONS + [(-0.5, 1e-7), (300.0, 0.25)]:
        want, absolute = U.ecc_sums(planes, tx, ty)
        got = ai.ecc_sums(device_planes, tx, ty)
        again = ai.ecc_sums(device_planes, tx, ty)
        assert got.tobytes() == again.tobytes()
        bound = n * 2.0 ** -53 * absolute
        for k, name in enumerate(U.SUM_NAMES):
            print(shape, (tx, ty), name, got[k], want[k], bound[k])
            assert abs(got[k] - want[k]) <= bound[k], (shape, (tx, ty), name, got[k], want[k], bound[k])
        assert got[0] == want[0]


@pytest.mark.parametrize("k", range(len(SHAPES)))
def test_translation_against_the_restatement_and_the_truth(ai, dev, recorded, k):
    shape = SHAPES[k]
    assert tuple(recorded["ecc_shapes"][k]) == shape
    tmpl, subj, truth, _ = case(shape)
    want_tx, want_ty, _, want_count, status = restated_run(shape)
    assert status == U.ECC_OK
    a, b = to_dev(tmpl, dev), to_dev(subj, dev)
    tx, ty, rho, count = ai.ecc_translation(a, b)
    print(shape, "device", tx, ty, rho, count, "restatement", want_tx, want_ty, want_count, "truth", truth)
    assert abs(tx - want_tx) <= 1e-3 and abs(ty - want_ty) <= 1e-3
    allowed = float(recorded["ecc_error"][k]) + 1e-3
    assert abs(tx - truth[0]) <= allowed and abs(ty - truth[1]) <= allowed
    assert abs(count - want_count) <= 1
    # the batch size changes how often the state is read, not the iterate
    for batch in (1, 7):
        assert ai.ecc_translation(a, b, batch=batch) == (tx, ty, rho, count)
    # fewer iterations than it needs: stops on the count
    assert ai.ecc_translation(a, b, iterations=3)[3] == 3
    m = ai.get_transformation_matrix(a, b, verbose=False)
    assert m.dtype == np.float32 and m.shape == (3, 3)
    assert np.array_equal(m, np.linalg.inv(np.array([[1, 0, tx], [0, 1, ty], [0, 0, 1]], np.float32)))


def test_failure_statuses_raise_and_the_library_stays_usable(ai, dev):
    flat = to_dev(np.full((20, 24), 7.0, np.float32), dev)
    with pytest.raises(RuntimeError, match="NaN encountered"):
        ai.get_transformation_matrix(flat, flat, verbose=False)
    a = U.smooth_plane((20, 24), 3)()
    with pytest.raises(RuntimeError, match="NaN encountered"):
        ai.ecc_translation(to_dev(a, dev), to_dev(a, dev), start=(40.0, 0.0))     # the shift empties the mask
    with pytest.raises(RuntimeError, match="The correlation is going to be minimized"):
        ai.ecc_translation(to_dev(a, dev), to_dev((300 - a).astype(np.float32), dev))
    from ipp_amd import capi
    with pytest.raises(capi.MiError):
        ai.ecc_translation(to_dev(a[:2], dev), to_dev(a[:2], dev))                # fewer than three rows
    tx, ty, rho, _ = ai.ecc_translation(to_dev(a, dev), to_dev(a, dev))
    assert abs(tx) < 1e-6 and abs(ty) < 1e-6 and rho > 0.999999


def test_align_images_moves_equal_the_restatement(ai, dev, recorded):
    """The fixture keeps every pre-rounding sum of the restatement at least 0.1 from a half-integer (asserted when the golden file
    is made), so the 1e-3 pixel between the two ECCs cannot flip ``round``: the moves are equal as integers."""
    assert recorded["align_margin"] >= 0.1
    ref, sub = U.blob_volume(seed=int(recorded["align_seed"]))
    img1, img2 = to_dev(ref, dev), to_dev(sub, dev)
    x, y, z, residual = ai.align_images(img1, img2, 10)
    print("moves", x, y, z, "residual", residual)
    want = recorded["align_moves"]
    assert [x, y, z] == want.tolist()
    assert [sum(x), sum(y), sum(z)] == want.sum(axis=1).tolist() == [-3, 2, -1]
    assert residual is not None and all(np.isfinite(r) for r in residual)
    # img2 was moved in place by the total, img1 not at all
    moved = sub.copy()
    for axis, moves in ((2, x), (1, y), (0, z)):
        for m in moves:
            U.roll_pad(moved, m, axis=axis)
    assert np.array_equal(ai._host(img2), moved) and np.array_equal(ai._host(img1), ref)
    # make_copy leaves both alone; align_all_images sums the moves and skips the reference
    img2 = to_dev(sub, dev)
    moves, residuals = ai.align_all_images([img1, None, img2], reference=0, max_iter=10, make_copy=True)
    assert moves == [[None] * 3, [None] * 3, [-3, 2, -1]] and residuals[0] is None and residuals[1] is None
    assert np.array_equal(ai._host(img2), sub)


@pytest.mark.parametrize("src", [np.uint8, np.uint16])
@pytest.mark.parametrize("name", list(U.COMPOSITE_CASES))
def test_composite_equals_the_numpy_steps(ai, dev, name, src):
    shapes, reference, offsets = U.COMPOSITE_CASES[name]
    volumes = U.composite_volumes(shapes, src)
    maps = ai.composite_index_map(shapes, reference, offsets)
    nz, ny, nx = shapes[reference]
    whole = [None if v is None else to_dev(v, dev) for v in volumes]
    for out in ("uint8", "uint16", "uint32", "float32"):
        want = U.composite(volumes, reference, offsets, out)
        got = ai._host(ai.channel_composite(whole, [0, 0, 0], maps, 0, nz, (ny, nx), out))
        assert got.dtype == want.dtype and np.array_equal(got, want), (name, out)
        # in groups, each channel handed over as the slices the group needs and no others
        for z0, n in ((0, 1), (1, nz - 1)):
            sources, firsts = [], []
            for c, v in enumerate(volumes):
                a, b = (0, 0) if v is None else (max(0, z0 + maps[c][0]), min(v.shape[0], z0 + n + maps[c][0]))
                firsts.append(a)
                sources.append(to_dev(v[a:b], dev) if b > a else None)
            if all(s is None for s in sources):
                continue
            got = ai._host(ai.channel_composite(sources, firsts, maps, z0, n, (ny, nx), out))
            assert np.array_equal(got, want[z0:z0 + n]), (name, out, z0, n)


def _tree(folder):
    return {str(p.relative_to(folder)): (hashlib.sha256(p.read_bytes()).hexdigest(), p.stat().st_mtime_ns)
            for p in sorted(folder.rglob("*")) if p.is_file()}


def test_main_on_a_folder_of_three_channels(ai, dev, recorded, tmp_path):
    from ipp_amd import brickio
    assert recorded["main_margin"] >= 0.1
    down, orig = U.main_fixture(int(recorded["main_seed"]))
    names = ("red", "green", "blue")
    for kind, volumes in (("orig", orig), ("down", down)):
        for name, v in zip(names, volumes):
            brickio.save_tiff_series(tmp_path / kind / name, v, compression=None)
    inputs = {n: (str(tmp_path / "orig" / n), str(tmp_path / "down" / n)) for n in names}
    out = tmp_path / "out"
    args = Namespace(**inputs, output=str(out), max_iterations=10, write_alignments=True, reference="red", num_threads=4, generate_ims=False,
                     save_singles=False, dtype="uint32", dx=(1, 2), dy=(1, 2), dz=(1, 1))
    alignments, residuals = ai.main(args)

    want_moves = [[None if v == -1000 else int(v) for v in row] for row in recorded["main_alignments"]]
    assert alignments == want_moves
    for got, want in zip(residuals, recorded["main_residuals"]):
        assert (got is None) == bool(np.isnan(want[0]))
        if got is not None:
            assert np.all(np.abs(np.array(got, np.float64) - want) <= 1e-3), (got, want)
    want = U.main_arrays(down, orig, 0, want_moves, "uint32", (1, 2), (1, 2), (1, 1))
    # x and y at half the down-sampled voxel size move twice as far, z as far; (z, y, x) order
    assert want["scaled"] == [[0, 0, 0]] + [[a[2], 2 * a[1], 2 * a[0]] for a in want_moves[1:]]

    files = sorted((out / "downsampled" / "RGB").iterdir(), key=lambda p: int(p.stem))
    assert [p.name for p in files] == [f"{k}.tif" for k in range(down[0].shape[0])]
    got = np.stack([U.read_tiff(p)[0] for p in files])
    assert got.dtype == np.uint32 and np.array_equal(got, want["down_rgb"])
    files = sorted((out / "original" / "RGB").iterdir())
    assert [p.name for p in files] == [f"img_{k + 1:06d}.tif" for k in range(orig[0].shape[0])]
    got = np.stack([U.read_tiff(p)[0] for p in files])
    assert got.dtype == np.uint16 and np.array_equal(got, want["orig_rgb"])      # kept: the original series has the slices' own dtype
    downsampled_input = tuple(inputs[n][1] for n in names)
    assert (out / "alignments.txt").read_text() == U.alignments_text(want_moves, downsampled_input, residuals, 0)

    before = _tree(out)
    ai.main(Namespace(**dict(vars(args), write_alignments=False)))
    assert _tree(out) == before
