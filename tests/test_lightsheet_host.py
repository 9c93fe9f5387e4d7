"""CPU: the lightsheet correction without a device -- the restatement of tests/lightsheet_util.py against the goldens of the
reference's own code (tests/golden/lightsheet, made by tests/golden/make_lightsheet_golden.py), its resampling against
scipy.ndimage.zoom, ``mi_lightsheet_derive`` against the restatement's bookkeeping, and the refusals."""
import glob
import json
import os

import numpy as np
import pytest

from tests import lightsheet_util as L
from tests.conftest import ROOT

GOLD = os.path.join(ROOT, "tests", "golden", L.GOLDEN_SUBDIR)
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLD, "*.npz")) if not p.endswith("_maps.npz"))


def load_case(name):
    z = dict(np.load(os.path.join(GOLD, name + ".npz")))
    maps = os.path.join(GOLD, name + "_maps.npz")
    if os.path.exists(maps):
        z.update(np.load(maps))
    kwargs = json.loads(str(z["kwargs"]))
    if kwargs.get("down_sample") is not None:
        kwargs["down_sample"] = tuple(kwargs["down_sample"])
    return z, kwargs, str(z["kind"])


CORRECT = [c for c in CASES if not c.startswith("pi_")]
PROCESS = [c for c in CASES if c.startswith("pi_")]


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


def test_goldens_are_present():
    assert len(CORRECT) == 17 and len(PROCESS) == 7
    for p in glob.glob(os.path.join(GOLD, "*.npz")):
        assert os.path.getsize(p) < 1 << 20, p


@pytest.mark.parametrize("name", CORRECT)
def test_restatement_equals_the_reference(name):
    z, kw, kind = load_case(name)
    assert kind == "correct"
    got = L.correct_lightsheet(z["img"].copy(), **kw)
    for g, what in zip(got, ("out", "ls", "bg", "ls_grid", "bg_grid")):
        assert g.dtype == z[what].dtype and np.array_equal(g, z[what]), what   # integer tiles: equal; float32: to the last bit


@pytest.mark.parametrize("name", PROCESS)
def test_restated_process_img_equals_the_reference(name):
    z, kw, kind = load_case(name)
    assert kind == "process"
    got = L.process_img(z["img"].copy(), flat=z.get("flat"), **kw)
    assert got.dtype == z["out"].dtype and np.array_equal(got, z["out"])


def test_goldens_show_the_quirks():
    z, _, _ = load_case("u16_300x634_zero_lines")
    assert not z["bg"][-1].any() and not z["bg"][:, -1].any() and not z["ls"][:, -1].any() and z["ls"][-1, :-1].any()
    assert np.array_equal(z["out"][-1], z["img"][-1]) and np.array_equal(z["out"][:, -1], z["img"][:, -1])   # left uncorrected
    z, _, _ = load_case("u16_130x310_wrap")
    assert z["bg"].min() > 32767      # bg * 2 wraps modulo 2^16
    wrapped = np.minimum(z["img"], np.minimum(z["ls"], (z["bg"].astype(np.int64) * 2 % 65536).astype(np.uint16)))
    assert np.array_equal(z["out"], z["img"] - wrapped)
    a, _, _ = load_case("u16_factor_2p9")
    assert np.array_equal(a["out"], L.correct_lightsheet(a["img"].copy(), lightsheet_vs_background=2.0)[0])   # 2.9 truncates to 2
    f, _, _ = load_case("f32_factor_2p9")
    assert not np.array_equal(f["out"], L.correct_lightsheet(f["img"].copy(), lightsheet_vs_background=2.0)[0])


def test_row_windows_vectorised_like_the_loop():
    """numpy.percentile over an axis does the arithmetic of the per-window calls (used for the big GPU cases)."""
    for dt in (np.uint16, np.float32):
        img = L.bead_and_stripe_tile((40, 700), 5, dt)
        for length, p in ((150, 0.25), (64, 0.03), (151, 0.5)):
            assert np.array_equal(L.row_grid(img, p, length), L.percentile_grid(img, p, (1, length)))


@pytest.mark.parametrize("n_in,n_out", [(7, 188), (8, 205), (12, 300), (25, 634), (4, 611), (4, 634), (7, 1093), (40, 1024), (81, 2048),
                                        (1, 150), (13, 2048), (5, 128), (1, 25), (3, 3)])
def test_restated_resampling_equals_scipy(n_in, n_out):
    from scipy.ndimage import zoom
    rng = np.random.default_rng(n_in * 10007 + n_out)
    quirk = bool(L.zoom_axis(n_in, n_out)[3][-1])
    assert quirk == ((n_in, n_out) in [(7, 188), (8, 205), (12, 300), (25, 634), (4, 611), (4, 634), (7, 1093)])
    other_in, other_out = 6, 97
    for grid in (rng.integers(0, 65536, (n_in, other_in)).astype(np.uint16), rng.integers(0, 256, (other_in, n_in)).astype(np.uint8),
                 (rng.random((n_in, other_in)) * 3000).astype(np.float32)):
        shape = (n_out, other_out) if grid.shape[0] == n_in else (other_out, n_out)
        want = zoom(grid, tuple(float(s) / float(r) for s, r in zip(shape, grid.shape)), order=1)
        got = L.zoom1(grid, shape)
        assert got.dtype == want.dtype and np.array_equal(got, want)
        if quirk:
            assert not (got[-1] if grid.shape[0] == n_in else got[:, -1]).any()


SHAPES = [(301, 457), (128, 150), (130, 310), (300, 634), (25, 150), (49, 1897), (608, 170), (97, 331), (257, 449), (213, 600),
          (2048, 2048), (15000, 20000)]


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("length,window", [(150, 200), (64, 100), (151, 51)])
def test_derive_equals_the_restatement(ps, shape, length, window):
    from ipp_amd import capi
    prm = ps.make_lightsheet_params(np.uint16, length, window)
    if shape[1] < length:      # no lightsheet centre: refused, not a division by zero
        with pytest.raises(capi.MiError, match="no centre"):
            ps.derive_lightsheet(shape, np.uint16, prm)
        return
    info = ps.derive_lightsheet(shape, np.uint16, prm)
    want = L.bookkeeping(shape, length, window)
    got = {k: getattr(info, k) for k in want}
    assert got == want
    assert (info.ny, info.nx) == shape and info.integer_mode == 1
    cells = info.ls_ny * info.ls_nx + info.bg_ny * info.bg_nx
    assert 2 * cells <= info.scratch_bytes_per_tile <= 2 * cells + 32
    assert ps.derive_lightsheet(shape, np.float32, prm).integer_mode == 0


def test_derive_refuses_what_is_not_built(ps):
    from ipp_amd import capi
    for kw, code in ((dict(background_window_size=300), capi.MI_ERR_UNSUPPORTED),    # 150 x 150 samples after the step
                     (dict(artifact_length=5000), capi.MI_ERR_UNSUPPORTED)):
        with pytest.raises(capi.MiError) as e:
            ps.derive_lightsheet((6000, 6000), np.uint16, ps.make_lightsheet_params(np.uint16, **kw))
        assert e.value.code == code
    info = ps.derive_lightsheet((2048, 2048), np.uint16, ps.make_lightsheet_params(np.uint16, background_window_size=256))
    assert info.max_window_samples == 128 * 128      # the largest window that is built for every type
    with pytest.raises(capi.MiError):                # no centre fits: the C side says so too
        ps.derive_lightsheet((20, 400), np.uint16, ps.make_lightsheet_params(np.uint16))


def test_refusals_name_the_option(ps):
    for shape in ((8, 8), (100, 149), (24, 400), (400, 24)):
        with pytest.raises(NotImplementedError, match="lightsheet"):
            ps.process_img(np.zeros(shape, np.uint16), lightsheet=True)          # uniform AND too small: the shape decides first
    with pytest.raises(NotImplementedError, match="lightsheet"):
        ps.process_img(np.zeros((40, 320), np.uint16), lightsheet=True, down_sample=(2, 2))     # 20 x 160 after down-sampling
    tile = np.zeros((64, 300), np.uint16)
    with pytest.raises(NotImplementedError, match="mask"):
        ps.correct_lightsheet(tile, mask=np.ones_like(tile, bool))
    with pytest.raises(NotImplementedError, match="mask"):
        ps.local_percentile(tile, 0.25, mask=np.ones_like(tile, bool))
    with pytest.raises(NotImplementedError, match="selem"):
        ps.local_percentile(tile, 0.25, selem=np.ones((3, 3), bool))
    with pytest.raises(NotImplementedError, match="percentile"):
        ps.local_percentile(tile, [0.25, 0.5])
    with pytest.raises(NotImplementedError, match="interpolate"):
        ps.local_percentile(tile, 0.25, interpolate=2)
    with pytest.raises(NotImplementedError, match="percentile"):
        ps.make_lightsheet_params(np.uint16, percentile=(0.1, 0.2))
    with pytest.raises(ValueError, match="Percentiles"):
        ps.make_lightsheet_params(np.uint16, percentile=1.5)
    # the other refusals of process_img stay
    for kw, word in ((dict(new_size=(4, 4)), "new_size"), (dict(bleach_correction_frequency=0.01), "bleach_correction_frequency")):
        with pytest.raises(NotImplementedError, match=word):
            ps.process_img(np.zeros((64, 300), np.uint16), lightsheet=True, **kw)


def test_command_line_takes_the_lightsheet_options(ps):
    a = ps._parse_args(["--input", "x", "--lightsheet", "--artifact_length", "64", "--background_window_size", "100", "--percentile", "0.3",
                        "--lightsheet_vs_background", "2.9"])
    assert (a.lightsheet, a.artifact_length, a.background_window_size, a.percentile, a.lightsheet_vs_background) == (True, 64, 100, 0.3, 2.9)
    d = ps._parse_args(["--input", "x"])
    assert (d.lightsheet, d.artifact_length, d.background_window_size, d.percentile, d.lightsheet_vs_background) == (False, 150, 200, 0.25, 2.0)
