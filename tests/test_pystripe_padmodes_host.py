"""CPU: the value padding modes of the pystripe stage (constant / linear_ramp / maximum / mean / median / minimum): what the Python
layer takes and refuses, what the plan's bookkeeping holds for them, how the acquisition driver hands the mode on, and the restatement
of tests/pystripe_pad_util.py against numpy's corner rule written out by hand."""
import math

import numpy as np
import pytest

from tests import acquisition_util as AU
from tests import pystripe_pad_util as PU


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


def test_make_params_takes_the_six_modes_with_extended(ps):
    from ipp_amd import capi
    codes = dict(constant=4, linear_ramp=5, maximum=6, mean=7, median=8, minimum=9)
    assert capi.PS_VALUE_PADDING == PU.VALUE_MODES and {m: capi.PS_PADDING[m] for m in PU.VALUE_MODES} == codes
    assert [capi.PS_PADDING[m] for m in PU.INDEX_MODES] == [0, 1, 2, 3]
    for mode in PU.VALUE_MODES:
        p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode=mode, extended=True)
        assert p.padding_mode == codes[mode] and p.bleach_clip_min == 0.0
        assert ps.make_params(np.uint16, sigma=(8, 8), padding_mode=mode.upper(), extended=True).padding_mode == codes[mode]
        with pytest.raises(NotImplementedError, match="padding_mode"):
            ps.make_params(np.uint16, sigma=(8, 8), padding_mode=mode)
    # the constant travels as the clip itself (the C side pads with log1p of it), with and without a frequency; not for another
    # mode; NaN for an estimated minimum.  The struct has no field of its own for it
    assert [f[0] for f in capi.PystripeParams._fields_][-1] == "bleach_max_method"
    p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bleach_correction_clip_min=5.3, extended=True)
    assert p.bleach_clip_min == 5.3 and p.bleach_frequency == 0.0 and p.bleach_auto == 0
    p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bleach_correction_frequency=0.01, bleach_correction_clip_min=5.3,
                       bleach_correction_clip_med=6.0, bleach_correction_clip_max=7.0, extended=True)
    assert p.bleach_clip_min == 5.3 and p.bleach_frequency == 0.01
    p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="mean", bleach_correction_clip_min=5.3, extended=True)
    assert p.bleach_clip_min == 0.0
    p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bleach_correction_frequency=0.01, extended=True)
    assert math.isnan(p.bleach_clip_min) and p.bleach_auto == 7
    with pytest.raises(ValueError, match="bleach_correction_clip_min"):
        ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bleach_correction_clip_min=-0.5, extended=True)
    # two plans that differ in the constant alone are two plans
    a = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", extended=True)
    b = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bleach_correction_clip_min=1.0, extended=True)
    assert ps.plan_key((64, 64), np.uint16, a) != ps.plan_key((64, 64), np.uint16, b)


def test_empty_is_refused_with_and_without_extended(ps):
    for extended in (False, True):
        with pytest.raises(NotImplementedError, match="padding_mode='empty'"):
            ps.make_params(np.uint16, sigma=(8, 8), padding_mode="empty", extended=extended)
        with pytest.raises(NotImplementedError, match="padding_mode"):
            ps.process_img(np.zeros((40, 40), np.uint16), sigma=(8, 8), wavelet="db9", padding_mode="empty", extended=extended)
    with pytest.raises(RuntimeError, match="padding_mode"):
        ps.make_params(np.uint16, sigma=(8, 8), padding_mode="bogus", extended=True)


def test_clip_min_reaches_make_params_without_a_frequency(ps):
    assert ps._bleach_opts((64, 64), None, None, False, None, 6.0, 7.0) == {}
    assert ps._bleach_opts((64, 64), None, None, False, 5.3, 6.0, 7.0) == dict(bleach_correction_clip_min=5.3)
    p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", extended=True, **ps._bleach_opts((64, 64), None, None, True, 5.3, None, None))
    assert p.bleach_clip_min == 5.3 and p.bleach_frequency == 0.0


def test_scratch_grows_by_the_padded_image_in_a_value_mode_only(ps):
    shape = (97, 128)
    info = {m: ps.derive(shape, np.uint16, ps.make_params(np.uint16, sigma=(8, 8), padding_mode=m, bidirectional=True, extended=True))
            for m in PU.INDEX_MODES + PU.VALUE_MODES}
    base = info["reflect"].scratch_bytes_per_tile
    i = info["reflect"]
    ny, nx, image = i.ny, i.nx, i.padded_ny * i.padded_nx
    assert (i.padded_ny, i.padded_nx) == (97 + 2 * i.base_pad + 1, 128 + 2 * i.base_pad) and i.levels >= 1

    def floats(n):   # the scratch is handed out in units of four floats
        return (n + 3) // 4 * 4

    for m in PU.INDEX_MODES:
        assert info[m].scratch_bytes_per_tile == base, m
    grown = {m: (info[m].scratch_bytes_per_tile - base) // 4 for m in PU.VALUE_MODES}
    vectors, partials = floats(ny + nx + 1), floats(2 * ny * ((nx + 63) // 64))
    assert grown == dict(constant=floats(image), linear_ramp=floats(image), median=floats(image) + vectors,
                         maximum=floats(image) + vectors + partials, minimum=floats(image) + vectors + partials,
                         mean=floats(image) + vectors + partials)
    # a two-pass plan holds the padded image already; a constant with an estimated minimum holds that minimum per tile
    two = {m: ps.derive(shape, np.uint16, ps.make_params(np.uint16, sigma=(6, 20), padding_mode=m, extended=True)).scratch_bytes_per_tile
           for m in ("reflect", "constant", "linear_ramp")}
    assert two["reflect"] == two["constant"] == two["linear_ramp"]
    auto = ps.derive(shape, np.uint16, ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bidirectional=True,
                                                      bleach_correction_frequency=1 / 32, extended=True)).scratch_bytes_per_tile
    given = ps.derive(shape, np.uint16, ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", bidirectional=True,
                                                       bleach_correction_frequency=1 / 32, bleach_correction_clip_min=1.0,
                                                       bleach_correction_clip_med=2.0, bleach_correction_clip_max=3.0,
                                                       extended=True)).scratch_bytes_per_tile
    assert auto - given == 4 * floats(1)


def test_c_abi_names_padding_mode_for_a_code_out_of_range(ps):
    import ctypes as C
    from ipp_amd import capi
    for code in (-1, 10, 77):
        p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="reflect")
        p.padding_mode = code
        info = capi.PystripeInfo()
        rc = capi.lib().mi_pystripe_derive(64, 64, capi.PS_U16, C.byref(p), C.byref(info))
        assert rc == capi.MI_ERR_INVALID
        with pytest.raises(Exception, match="padding_mode"):
            capi.check(rc)
    # constant without a frequency pads with log1p(bleach_clip_min): a NaN or a negative clip is named
    for clip in (math.nan, -0.5):
        p = ps.make_params(np.uint16, sigma=(8, 8), padding_mode="constant", extended=True)
        p.bleach_clip_min = clip
        rc = capi.lib().mi_pystripe_derive(64, 64, capi.PS_U16, C.byref(p), C.byref(info))
        assert rc == capi.MI_ERR_INVALID
        with pytest.raises(Exception, match="bleach_clip_min"):
            capi.check(rc)


def test_acquisition_carries_the_mode_into_process_img(tmp_path):
    from ipp_amd import acquisition as A
    for name in ("tmp", "out"):
        (tmp_path / name).mkdir()
    acq = tmp_path / "acq"
    AU.write_empty_acquisition(acq, AU.CHANNELS[:1], z_step=20)
    args = A.build_parser().parse_args(["--objective", "15x", "-i", str(acq), "-t", str(tmp_path / "tmp"), "-s", str(tmp_path / "out"),
                                        "--bleach_wavelet", "db9", "--padding_mode", "mean"])
    c = A.plan(args).channels[0]
    estimate = dict(bleach_correction_clip_min=5.25, bleach_correction_clip_med=6.5, bleach_correction_clip_max=8.75, bit_shift_to_right=3, dark=190)
    assert c.process_img_kwargs(estimate, (320, 318), "uint16")["padding_mode"] == "mean"


def test_restatement_follows_numpys_corner_rule():
    """3 x 4 by hand: axis 0 first, then axis 1 over all rows, the new ones included."""
    x = np.array([[1, 2, 3, 6], [4, 4, 8, 0], [7, 0, 1, 12]], np.float64)
    widths = ((2, 1), (1, 2))
    got = PU.pad_log(x, widths, "mean")
    col, row = x.mean(axis=0), x.mean(axis=1)          # [4, 2, 4, 6], [3, 4, 5]
    corner = col.mean()                                  # the mean of the column means: 4
    assert col.tolist() == [4, 2, 4, 6] and row.tolist() == [3, 4, 5] and corner == 4
    want = np.empty((6, 7))
    want[2:5, 1:5] = x
    want[[0, 1, 5], 1:5] = col
    want[2:5, 0], want[2:5, 5], want[2:5, 6] = row, row, row
    want[[0, 1, 5], 0] = want[[0, 1, 5], 5] = want[[0, 1, 5], 6] = corner
    assert np.array_equal(got, want)
    # linear_ramp from 0: a front pad of width p holds edge * k / p, a back pad of width q edge * (q - 1 - k) / q; axis 1 ramps the
    # ramped rows
    got = PU.pad_log(x, widths, "linear_ramp")
    rows = np.vstack([x[0] * 0 / 2, x[0] * 1 / 2, x, x[2] * 0 / 1])
    want = np.hstack([rows[:, :1] * 0 / 1, rows, rows[:, -1:] * 1 / 2, rows[:, -1:] * 0 / 2])
    assert np.allclose(got, want, rtol=0, atol=1e-15) and got[1, 5] == x[0, 3] / 2 / 2
    # the other statistics and the constant
    for mode, f in (("maximum", np.max), ("minimum", np.min), ("median", np.median)):
        got = PU.pad_log(x, widths, mode)
        assert np.array_equal(got[0, 1:5], f(x, axis=0)) and np.array_equal(got[2:5, 6], f(x, axis=1)) and got[5, 0] == f(f(x, axis=0))
    assert np.median(x, axis=1).tolist() == [2.5, 4, 4]   # an even count: the mean of the two middle values
    got = PU.pad_log(x.astype(np.float32), widths, "constant", PU.pad_constant(5.3))
    assert got.dtype == np.float32 and got[0, 0] == np.float32(math.log1p(5.3)) and PU.pad_constant(None) == 0.0
    assert PU.LDS_LINE == 9968
