"""GPU: the lightsheet correction (include/mi_lightsheet.h, ipp_amd.pystripe) against the goldens of the reference's own code
(tests/golden/lightsheet) and, for sizes the goldens cannot hold, against the restatement of tests/lightsheet_util.py.

The standard: integer tiles EQUAL the reference (output, lightsheet map, background map, both sub-grids).  float32 tiles: the
sub-grids (order statistics) equal the reference's; maps and output may be at most 4 x E_ref from the restatement's float64 run,
E_ref being the reference's own float32 distance from it (stored in the golden; the factor of DESIGN section 12).  That bound is
evaluated and printed; the device turned out bit-identical to the reference's float32 arrays on every golden,
so equality is asserted for them as well.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import lightsheet_util as L
from tests import pystripe_util as U
from tests.conftest import ROOT
from tests.test_lightsheet_host import CORRECT, PROCESS, load_case

pytestmark = pytest.mark.gpu
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)
INT_CORRECT = [c for c in CORRECT if not c.startswith("f32")]
F32_CORRECT = [c for c in CORRECT if c.startswith("f32")]


def report(line):
    print("[lightsheet] " + line, flush=True)


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


def correct_kwargs(kw):
    """correct_lightsheet's dictionaries for process_img's option names"""
    length, window = kw.get("artifact_length", 150), kw.get("background_window_size", 200)
    out = dict(lightsheet=dict(selem=(1, length, 1)),
               background=dict(selem=(window, window, 1), spacing=(25, 25, 1), interpolate=1, step=(2, 2, 1)))
    for k in ("percentile", "lightsheet_vs_background"):
        if k in kw:
            out[k] = kw[k]
    return out


def neighbours(img, n=5):
    """a stack with ``img`` in the middle of tiles of different content"""
    rolled = [np.roll(img, (7 * i + 3, 13 * i + 5), (0, 1)) for i in range(n)]
    rolled[n // 2] = img
    return np.stack(rolled)


@pytest.mark.parametrize("name", INT_CORRECT)
def test_integer_golden_equals_the_reference(ps, dev, name):
    import torch
    z, kw, _ = load_case(name)
    img = z["img"]
    ckw = correct_kwargs(kw)
    out, ls, bg = ps.correct_lightsheet(img.copy(), return_lightsheet=True, return_background=True, device=dev, **ckw)
    for got, what in ((out, "out"), (ls, "ls"), (bg, "bg")):
        assert got.dtype == z[what].dtype and np.array_equal(got, z[what]), what
    assert np.array_equal(ps.correct_lightsheet(img.copy(), device=dev, **ckw), z["out"])
    assert np.array_equal(ps.correct_lightsheet(img.copy(), return_background=True, device=dev, **ckw)[1], z["bg"])
    # device tensor in, device tensor out; the input is left alone
    t = torch.from_numpy(img).to(dev)
    got = ps.correct_lightsheet(t, return_lightsheet=True, **ckw)
    assert all(isinstance(g, torch.Tensor) and g.is_cuda for g in got)
    assert np.array_equal(got[0].cpu().numpy(), z["out"]) and np.array_equal(got[1].cpu().numpy(), z["ls"]) and np.array_equal(t.cpu().numpy(), img)
    # inside a stack of five different tiles
    stack = neighbours(img)
    so, sl, sb = ps.correct_lightsheet(stack, return_lightsheet=True, return_background=True, device=dev, **ckw)
    assert np.array_equal(so[2], z["out"]) and np.array_equal(sl[2], z["ls"]) and np.array_equal(sb[2], z["bg"])
    assert not np.array_equal(so[1], so[2])
    # the sub-grids
    length, window = kw.get("artifact_length", 150), kw.get("background_window_size", 200)
    p = kw.get("percentile", 0.25)
    assert np.array_equal(ps.local_percentile(img, p, selem=(1, length, 1), interpolate=None, device=dev), z["ls_grid"])
    assert np.array_equal(ps.local_percentile(img, p, selem=(window, window, 1), spacing=(25, 25, 1), step=(2, 2, 1), interpolate=None,
                                              device=dev), z["bg_grid"])
    assert np.array_equal(ps.local_percentile(torch.from_numpy(stack).to(dev), p, selem=(window, window), spacing=(25, 25), step=(2, 2),
                                              interpolate=1)[2].cpu().numpy(), z["bg"])
    # process_img with the same options
    assert np.array_equal(ps.process_img(img.copy(), lightsheet=True, device=dev, **kw), z["out"])
    assert np.array_equal(ps.process_img(torch.from_numpy(stack).to(dev), lightsheet=True, **kw)[2].cpu().numpy(), z["out"])


@pytest.mark.parametrize("name", [c for c in PROCESS if c != "pi_f32_flat"])
def test_integer_golden_through_process_img(ps, dev, name):
    import torch
    z, kw, _ = load_case(name)
    got = ps.process_img(z["img"].copy(), device=dev, **kw)
    assert got.dtype == z["out"].dtype and got.shape == z["out"].shape and np.array_equal(got, z["out"])
    stack = neighbours(z["img"])
    got = ps.process_img(torch.from_numpy(stack).to(dev), **kw)
    assert np.array_equal(got[2].cpu().numpy(), z["out"])


def float_check(label, got, want64, ref32, e_ref):
    """at most 4 x E_ref from the float64 result; equality when the reference itself is exact"""
    err = float(np.abs(got.astype(np.float64) - want64).max())
    same = bool(np.array_equal(got, ref32))
    report(f"{label}: device vs float64 {err:.3g}, E_ref {e_ref:.3g}, bit-identical to the reference's float32: {same}")
    assert got.dtype == np.float32
    if e_ref == 0:
        assert err == 0, label
    else:
        assert err <= 4 * e_ref, (label, err, e_ref)
    return same


@pytest.mark.parametrize("name", F32_CORRECT)
def test_float32_golden(ps, dev, name):
    z, kw, _ = load_case(name)
    img = z["img"]
    ckw = correct_kwargs(kw)
    out, ls, bg = ps.correct_lightsheet(img.copy(), return_lightsheet=True, return_background=True, device=dev, **ckw)
    o64, l64, b64 = L.correct_lightsheet(img.astype(np.float64), **kw)[:3]
    same = [float_check(f"{name} {what}", got, want, z[what], float(z["e_" + what]))
            for got, want, what in ((out, o64, "out"), (ls, l64, "ls"), (bg, b64, "bg"))]
    length, window = kw.get("artifact_length", 150), kw.get("background_window_size", 200)
    p = kw.get("percentile", 0.25)
    assert np.array_equal(ps.local_percentile(img, p, selem=(1, length, 1), interpolate=None, device=dev), z["ls_grid"])
    assert np.array_equal(ps.local_percentile(img, p, selem=(window, window, 1), spacing=(25, 25, 1), step=(2, 2, 1), interpolate=None,
                                              device=dev), z["bg_grid"])
    # measured bit-identical on the MI355X, so equality is the standard here as well
    assert all(same), same
    assert np.array_equal(ps.process_img(neighbours(img), lightsheet=True, device=dev, **kw)[2], z["out"])


def test_float32_golden_through_process_img_with_flat(ps, dev):
    z, kw, _ = load_case("pi_f32_flat")
    got = ps.process_img(z["img"].copy(), flat=z["flat"], device=dev, **kw)
    want64 = L.process_img(z["img"].astype(np.float64), flat=z["flat"], **kw)
    assert float_check("pi_f32_flat", got, want64, z["out"], float(z["e_out"]))    # bit-identical on the MI355X, like the cases above


def test_mixed_types_and_the_default_window(ps, dev):
    """What the goldens do not hold, against the restatement: an integer tile divided by a flat field (a float tile with integer maps
    from there on), d_type given, an integer factor, and correct_lightsheet's own default window (150, 1) along y."""
    img = L.bead_and_stripe_tile((257, 449), 40, np.uint16)
    img8 = L.bead_and_stripe_tile((257, 449), 44, np.uint8)
    flat = (0.5 + 0.5 * np.random.default_rng(41).random(img.shape)).astype(np.float32)
    for tile, kw in ((img, dict(flat=flat, flat_on_integers=True)), (img, dict(d_type="float32")), (img8, dict(d_type="uint16", dark=3)),
                     (img, dict(flat=flat, flat_on_integers=True, convert_to_16bit=True, rotate=270)), (img, dict(lightsheet_vs_background=1))):
        want = L.process_img(tile.copy(), **kw)
        got = ps.process_img(tile.copy(), lightsheet=True, device=dev, **{k: v for k, v in kw.items() if k != "flat_on_integers"})
        assert got.dtype == want.dtype and got.shape == want.shape, kw.keys()
        assert np.array_equal(got, want), kw.keys()
    tall = L.bead_and_stripe_tile((449, 257), 42, np.uint16)
    got = ps.correct_lightsheet(tall.copy(), return_lightsheet=True, device=dev)      # the reference's defaults: selem (150, 1, 1)
    ls = L.zoom1(L.percentile_grid(tall, 0.25, (150, 1)), tall.shape)
    bg = L.zoom1(L.percentile_grid(tall, 0.25, (200, 200), (25, 25), (2, 2)), tall.shape)
    assert np.array_equal(got[1], ls) and np.array_equal(got[0], L.combine(tall, ls, bg, 2.0))
    # windows up to 16384 samples after stepping, all three types; a plan with a long artifact window
    for dt in (np.uint8, np.uint16, np.float32):
        big = L.bead_and_stripe_tile((300, 1300), 43, dt)
        got = ps.local_percentile(big, 0.25, selem=(256, 256), spacing=(100, 100), step=(2, 2), interpolate=None, device=dev)
        assert np.array_equal(got, L.percentile_grid(big, 0.25, (256, 256), (100, 100), (2, 2))), dt
        got = ps.local_percentile(big, 0.25, selem=(1, 1024), interpolate=None, device=dev)
        assert np.array_equal(got, L.row_grid(big, 0.25, 1024)), dt


@pytest.mark.parametrize("kw", [dict(), dict(dark=60, convert_to_8bit=True, bit_shift_to_right=3, rotate=90, flip_upside_down=True),
                                dict(down_sample=(2, 2), artifact_length=64, background_window_size=100)])
def test_with_the_stripe_filter(ps, dev, kw):
    """The filter itself may differ from the reference by a count; the lightsheet step behind it may not: process_img(lightsheet=True)
    equals the restatement's step applied to the device's own result without it, then converted / flipped / rotated on the host."""
    img = U.synthetic_tile((301, 457), 50, np.uint16, "rows")
    filt = dict(sigma=(16, 16), **PIPE)
    tail = {k: kw[k] for k in ("convert_to_8bit", "bit_shift_to_right", "rotate", "flip_upside_down") if k in kw}
    head = {k: v for k, v in kw.items() if k not in tail and k not in ("artifact_length", "background_window_size")}
    ls_kw = {k: kw[k] for k in ("artifact_length", "background_window_size") if k in kw}
    got = ps.process_img(img.copy(), lightsheet=True, device=dev, **filt, **kw)
    before = ps.process_img(img.copy(), device=dev, **filt, **head)
    assert before.dtype == np.uint16
    want = L.process_img_tail(L.correct_lightsheet(before, **ls_kw)[0], d_type=np.uint16, **tail)
    assert got.dtype == want.dtype and np.array_equal(got, want)
    assert not np.array_equal(L.process_img_tail(before, d_type=np.uint16, **tail), want)


def equal_to_restatement(ps, dev, img, label):
    import time
    t0 = time.perf_counter()
    want, ls, bg = L.correct_lightsheet(img, fast_rows=True)[:3]
    t1 = time.perf_counter()
    got = ps.correct_lightsheet(img, return_lightsheet=True, return_background=True, device=dev, lightsheet=dict(selem=(1, 150, 1)))
    report(f"{label}: restatement {t1 - t0:.1f} s on the CPU")
    assert np.array_equal(got[1], ls) and np.array_equal(got[2], bg) and np.array_equal(got[0], want)
    assert np.array_equal(ps.process_img(img.copy(), lightsheet=True, device=dev), want)


def test_size_2048_uint16(ps, dev):
    equal_to_restatement(ps, dev, L.bead_and_stripe_tile((2048, 2048), 60, np.uint16), "2048 x 2048 uint16")


def test_size_1000x2303_uint8(ps, dev):
    equal_to_restatement(ps, dev, L.bead_and_stripe_tile((1000, 2303), 61, np.uint8), "1000 x 2303 uint8")


def test_size_4100x6150_uint16_slice(ps, dev):
    """One merged slice (the restatement needs about half a minute for it; a plain test function, so it runs once)."""
    equal_to_restatement(ps, dev, L.bead_and_stripe_tile((4100, 6150), 62, np.uint16), "4100 x 6150 uint16")


def test_batch_past_2_to_31_samples(ps, dev):
    """2050 tiles of 1024 x 1024 uint8 (2^31 + 2^21 samples) through ONE launch per kernel, in place: the tile offsets inside the
    kernels pass 2^31 in the image.  The first and the last tile equal the restatement; the zero tiles between them stay zero."""
    import torch
    n, ny, nx = 2050, 1024, 1024
    first, last = L.bead_and_stripe_tile((ny, nx), 70, np.uint8), L.bead_and_stripe_tile((ny, nx), 71, np.uint8)
    tin = torch.zeros((n, ny, nx), dtype=torch.uint8, device=dev)
    tin[0], tin[n - 1] = torch.from_numpy(first).to(dev), torch.from_numpy(last).to(dev)
    assert tin.numel() > 2 ** 31
    plan = ps.LightsheetPlan(dev, (ny, nx), np.uint8, ps.make_lightsheet_params(np.uint8, max_batch=n))
    assert plan.info.max_batch == n
    out, _, _ = plan.run(tin)
    torch.cuda.synchronize(dev)
    plan.close()
    assert out.data_ptr() == tin.data_ptr()
    assert np.array_equal(out[0].cpu().numpy(), L.correct_lightsheet(first, fast_rows=True)[0])
    assert np.array_equal(out[n - 1].cpu().numpy(), L.correct_lightsheet(last, fast_rows=True)[0])
    assert not bool(out[1:n - 1].any())
    del out, tin
    from ipp_amd import capi
    capi.release_cached_memory()


def _write_tiff(path, img):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(img).save(path, format="TIFF", compression="tiff_adobe_deflate")


def _read_tiff(path):
    from PIL import Image
    with Image.open(path) as im:
        return np.array(im)


def test_batch_filter_and_command_line(ps, dev, tmp_path):
    src, dst, dst2 = tmp_path / "in", tmp_path / "out", tmp_path / "out_cli"
    tiles = {f"ch0/000100/000100_{i:03d}.tif": L.bead_and_stripe_tile((130, 310), 80 + i, np.uint16) for i in range(4)}
    tiles.update({f"ch0/000200/t_{i:03d}.tif": L.bead_and_stripe_tile((97, 331), 90 + i, np.uint16) for i in range(2)})
    for rel, img in tiles.items():
        _write_tiff(src / rel, img)
    kw = dict(lightsheet=True, convert_to_8bit=True, bit_shift_to_right=2, artifact_length=64, background_window_size=100, percentile=0.3,
              lightsheet_vs_background=1.5)
    stats = {}
    assert ps.batch_filter(src, dst, device=dev, stats=stats, **kw) == 0
    assert stats["written"] == 6
    for rel, img in tiles.items():
        got = _read_tiff(dst / rel)
        one = ps.process_img(img.copy(), device=dev, **kw)
        assert got.dtype == np.uint8 and np.array_equal(got, one), rel
        assert np.array_equal(one, L.process_img(img.copy(), **kw)), rel
    # the command line in a process of its own
    cli = os.path.join(ROOT, "image-preprocessing-pipeline_amd", "pystripe.py")
    run = subprocess.run([sys.executable, cli, "--input", str(src), "--output", str(dst2), "--lightsheet", "--convert_to_8bit",
                          "--bit_shift_to_right", "2", "--artifact_length", "64", "--background_window_size", "100", "--percentile", "0.3",
                          "--lightsheet_vs_background", "1.5"], capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout + run.stderr
    for rel in tiles:
        assert np.array_equal(_read_tiff(dst2 / rel), _read_tiff(dst / rel)), rel
    # a folder with a tile too small for one window: refused by name
    _write_tiff(src / "ch0/000300/small.tif", np.zeros((20, 100), np.uint16))
    with pytest.raises(NotImplementedError, match="lightsheet"):
        ps.batch_filter(src, tmp_path / "out3", device=dev, lightsheet=True)
