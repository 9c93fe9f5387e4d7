"""CPU: the wavelets of the stripe filter (ipp_amd.wavelets, the ``wavelet=`` argument of ipp_amd.pystripe, mi_pystripe_derive_wavelet):
the built-in Daubechies family, what is accepted and refused, the plan key, the bookkeeping for any tap count, the command line."""
import ctypes as C
import math

import numpy as np
import pytest

from oracle import destripe_oracle as O
from tests import wavelet_util as W


@pytest.fixture(scope="module")
def ps():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import pystripe
    return pystripe


@pytest.fixture(scope="module")
def wv(ps):
    from ipp_amd import wavelets
    return wavelets


def test_daubechies_known_answers(wv):
    assert np.array_equal(wv.daubechies(1), np.array([1.0, 1.0]) / math.sqrt(2.0))
    r3 = math.sqrt(3.0)
    closed = np.array([1 + r3, 3 + r3, 3 - r3, 1 - r3]) / (4 * math.sqrt(2.0))
    assert np.abs(wv.daubechies(2) - closed).max() <= 1e-14
    assert np.abs(wv.daubechies(9) - O.db_filters(9)[2]).max() <= 1e-12
    for n in range(1, 21):
        h = wv.daubechies(n)
        assert len(h) == 2 * n
        assert W.orthonormality_residual(h) <= 1e-10, n
        assert wv.orthonormality_residual(h) == pytest.approx(W.orthonormality_residual(h), abs=1e-15)
        assert abs(h.sum() - math.sqrt(2.0)) <= 1e-12


def test_lattice_filter_is_orthonormal():
    for taps in (2, 8, 38, 90, 128):
        h = W.lattice_filter(taps, 3)
        assert len(h) == taps and W.orthonormality_residual(h) <= 1e-14 and abs(h.sum() - math.sqrt(2.0)) <= 1e-14
    assert not np.array_equal(W.lattice_filter(90, 1), W.lattice_filter(90, 2))
    # perfect reconstruction through the transform of the restatement, also where the extension reflects more than once
    F = W.filters_from_rec_lo(W.lattice_filter(90, 5))
    for n in (400, 61):
        x = np.random.default_rng(n).standard_normal((1, n))
        a, d = O.dwt_axis(x, F[0], 1), O.dwt_axis(x, F[1], 1)
        back = O.idwt_axis(a, d, F[2], F[3], 2 * a.shape[1] - 90 + 2, 1)[:, :n]
        assert np.abs(back - x).max() <= 1e-13


def test_accepted_forms(ps, wv):
    mk = ps.make_params
    assert mk(np.uint16, sigma=(8, 8), wavelet="db9").wavelet is None            # the name: the library's own 18-tap route
    assert mk(np.uint16, sigma=(0, 0), wavelet="coif15").wavelet is None         # no filter: the argument is not looked at
    assert mk(np.uint16, sigma=(8, 8), wavelet="haar").wavelet.rec_lo == mk(np.uint16, sigma=(8, 8), wavelet="db1").wavelet.rec_lo
    assert mk(np.uint16, sigma=(8, 8), wavelet="DB4").wavelet.taps == 8
    assert mk(np.uint16, sigma=(8, 8), wavelet="db20").wavelet.taps == 40
    h = W.lattice_filter(90, 1)

    class Duck:
        rec_lo = list(h)
        name = "coif15"

    for form in (h, list(h), tuple(h), Duck(), ps.orthogonal_wavelet(h), h.astype(np.float32)):
        w = mk(np.uint16, sigma=(8, 8), wavelet=form).wavelet
        assert isinstance(w, wv.OrthogonalWavelet) and w.taps == 90
        assert np.abs(w.array() - h).max() <= 1e-7
    assert mk(np.uint16, sigma=(8, 8), wavelet=Duck()).wavelet.name == "coif15"
    # the 18 db9 values as an array are a wavelet like any other: the generic route
    assert mk(np.uint16, sigma=(8, 8), wavelet=wv.daubechies(9)).wavelet.taps == 18
    w = ps.orthogonal_wavelet(h, name="stand-in")
    with pytest.raises(Exception):
        w.rec_lo = ()                                                            # immutable
    assert isinstance(w.rec_lo, tuple)


def test_refused_forms(ps, wv):
    mk = ps.make_params
    for name in ("coif15", "sym8", "db21", "db38", "db0", "bior2.2", "db", ""):
        with pytest.raises(NotImplementedError, match="wavelet") as e:
            mk(np.uint16, sigma=(8, 8), wavelet=name)
        assert "rec_lo" in str(e.value) and "coefficients" in str(e.value)        # how to hand the wavelet in instead
    h = W.lattice_filter(90, 1)
    off = h.copy()
    off[17] += 1e-3
    bior_lo = np.array([-1, 2, 6, 2, -1, 0]) * math.sqrt(2.0) / 8                 # bior2.2's reconstruction-side low-pass, zero-padded
    bad = [h[:89], [], np.zeros(0), W.lattice_filter(130, 1), np.where(np.arange(90) == 3, np.nan, h), np.where(np.arange(90) == 3, np.inf, h),
           off, bior_lo, h.reshape(2, 45), 2.0 * h]
    for form in bad:
        with pytest.raises(ValueError, match="wavelet"):
            mk(np.uint16, sigma=(8, 8), wavelet=form)
        with pytest.raises(ValueError, match="wavelet"):
            ps.orthogonal_wavelet(form)
    # raised from the values alone by every entry point, before a device is looked for
    tile = np.zeros((40, 50), np.uint16)
    for call in (lambda **k: ps.filter_streaks(tile, sigma=(8, 8), **k), lambda **k: ps.process_img(tile, sigma=(8, 8), **k),
                 lambda **k: ps.batch_filter("no_such_folder", "out", sigma=(8, 8), **k)):
        with pytest.raises(NotImplementedError, match="wavelet"):
            call(wavelet="coif15")
        with pytest.raises(ValueError, match="wavelet"):
            call(wavelet=off)


def test_the_c_side_checks_too(ps):
    from ipp_amd import capi
    lib = capi.lib()
    p = ps.make_params(np.uint16, sigma=(8, 8), wavelet="db9")
    info = capi.PystripeInfo()
    for taps in (0, 1, 7, 130, -2):
        assert lib.mi_pystripe_derive_wavelet(64, 64, 1, C.byref(p), taps, C.byref(info)) == capi.MI_ERR_INVALID
        assert "taps" in capi.last_error()
    assert capi.PS_MAX_TAPS == 128


def test_plan_key_goes_by_value(ps, wv):
    h = W.lattice_filter(90, 1)
    a = ps.make_params(np.uint16, sigma=(8, 8), wavelet=h.copy())
    b = ps.make_params(np.uint16, sigma=(8, 8), wavelet=ps.orthogonal_wavelet(list(h), name="another name"))
    assert a.wavelet is not b.wavelet and a.wavelet == b.wavelet and hash(a.wavelet) == hash(b.wavelet)
    assert ps.plan_key((64, 80), np.uint16, a) == ps.plan_key((64, 80), np.uint16, b)
    assert len({ps.plan_key((64, 80), np.uint16, a): 1, ps.plan_key((64, 80), np.uint16, b): 2}) == 1
    other = ps.make_params(np.uint16, sigma=(8, 8), wavelet=W.lattice_filter(90, 2))
    by_name = ps.make_params(np.uint16, sigma=(8, 8), wavelet="db9")
    as_array = ps.make_params(np.uint16, sigma=(8, 8), wavelet=wv.daubechies(9))
    keys = {ps.plan_key((64, 80), np.uint16, q) for q in (a, other, by_name, as_array)}
    assert len(keys) == 4                                                        # 'db9' by name and by value are different routes
    assert ps.plan_key((64, 80), np.uint16, a) != ps.plan_key((64, 82), np.uint16, a)
    assert ps.plan_key((64, 80), np.uint16, a) != ps.plan_key((64, 80), np.uint16, ps.make_params(np.uint16, sigma=(8, 9), wavelet=h))


SHAPES = [((2048, 2048), (250, 250), 0), ((330, 421), (16, 16), 0), ((40, 50), (16, 16), 0), ((40, 50), (16, 16), 2), ((33, 70), (3, 3), 0),
          ((33, 70), (3, 3), 7), ((97, 130), (6, 14), 0), ((150, 150), (8, 8), 1), ((1, 1), (2, 2), 0)]


@pytest.mark.parametrize("taps", [2, 8, 38, 90, 128])
def test_bookkeeping_for_any_tap_count(ps, taps):
    level_zero = 0
    for shape, sigma, level in SHAPES:
        prm = ps.make_params(np.uint16, sigma=sigma, level=level, wavelet=W.lattice_filter(taps, 4), padding_mode="reflect", bidirectional=True)
        info = ps.derive(shape, np.uint16, prm)
        bp, py, px, padded, lev, shapes = W.geometry(shape, sigma, taps, level)
        assert (info.base_pad, info.pad_y, info.pad_x) == (bp, py, px)
        assert (info.padded_ny, info.padded_nx) == padded
        assert info.levels == lev
        assert [(info.coef_ny[i], info.coef_nx[i]) for i in range(lev)] == shapes
        assert (info.out_ny, info.out_nx) == shape
        level_zero += lev == 0
        if lev:
            assert info.scratch_bytes_per_tile >= 4 * (2 * max((h0 + 1) * w1 for (h0, _), (_, w1) in zip([padded] + shapes, shapes))
                                                       + sum(4 * h * w for h, w in shapes))
    if taps >= 90:
        assert level_zero >= 3          # (40, 50), (33, 70), (1, 1): a padded extent below taps - 1
    if taps == 2:
        assert W.geometry((33, 70), (3, 3), 2, 7)[5][-1][0] == 1                  # Haar, explicit levels: a line of one sample


def test_eighteen_taps_derive_like_db9(ps):
    from ipp_amd import capi, wavelets
    fields = [name for name, _ in capi.PystripeInfo._fields_]
    for shape, sigma, level in SHAPES + [((333, 517), (40, 80), 3)]:
        kw = dict(sigma=sigma, level=level, padding_mode="wrap", bidirectional=True, dark=3,
                  bleach_correction_frequency=0.01, bleach_correction_clip_min=1.0, bleach_correction_clip_med=2.0, bleach_correction_clip_max=3.0)
        if min(shape) <= 6:
            kw = {k: v for k, v in kw.items() if not k.startswith("bleach")}
        named = ps.derive(shape, np.uint16, ps.make_params(np.uint16, wavelet="db9", **kw))
        valued = ps.derive(shape, np.uint16, ps.make_params(np.uint16, wavelet=wavelets.daubechies(9), **kw))
        for f in fields:
            a, b = getattr(named, f), getattr(valued, f)
            assert (list(a) == list(b)) if hasattr(a, "__len__") else (a == b), (shape, f)
        assert named.levels >= 1


def test_command_line(ps, wv, tmp_path):
    base = ["--input", "in", "--sigma1", "8", "--sigma2", "8"]
    a = ps._parse_args(base + ["--wavelet", "db4"])
    assert a.wavelet == "db4" and a.wavelet_file is None and ps._cli_wavelet(a) == "db4"
    assert ps._cli_wavelet(ps._parse_args(base)) == "db9"
    h = W.lattice_filter(90, 6)
    np.save(tmp_path / "w.npy", h)
    (tmp_path / "w.txt").write_text("\n".join(repr(float(v)) for v in h) + "\n")
    (tmp_path / "w.csv").write_text(", ".join(repr(float(v)) for v in h))
    for name in ("w.npy", "w.txt", "w.csv"):
        a = ps._parse_args(base + ["--wavelet_file", str(tmp_path / name)])
        w = ps._cli_wavelet(a)
        assert isinstance(w, wv.OrthogonalWavelet) and w.rec_lo == tuple(h)
    with pytest.raises(SystemExit):
        ps._parse_args(base + ["--wavelet", "db4", "--wavelet_file", str(tmp_path / "w.npy")])
    (tmp_path / "bad.txt").write_text("0.5 0.5 0.5")
    with pytest.raises(ValueError, match="wavelet"):
        ps._cli_wavelet(ps._parse_args(base + ["--wavelet_file", str(tmp_path / "bad.txt")]))


def test_parallel_image_processor_hands_the_object_through(ps):
    from ipp_amd import parallel_image_processor as pip
    w = ps.orthogonal_wavelet(W.lattice_filter(8, 1))
    seen = {}

    def fun(img, **kwargs):
        seen.update(kwargs)
        return img

    assert pip._call(fun, np.zeros((2, 2)), None, dict(wavelet=w, sigma=(1, 1))) is not None
    assert seen["wavelet"] is w
    import pickle
    assert pickle.loads(pickle.dumps(w)) == w
