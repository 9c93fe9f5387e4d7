"""GPU: mi_edgetaper3d on every blur route (direct shell, whole-block FFT, six face slabs) against R.edgetaper_3d at the shapes
where csrc/edgetaper.hip and the direct engine's EPI_TAPER_SHELL epilogue take branches that no smaller block reaches: tiles
skipped on the plateau, rows longer than a stride of the blend, even PSF extents, tapers with a plateau of one sample or none,
and engines that a deconvolution plan keeps between blocks.  Cases, plateaus and tiles: tests/edgetaper_util.py (pinned on the
host by tests/test_edgetaper_util_host.py).

Every call goes through the C ABI with a `work` volume that the test owns and fills with NaN: a voxel of `work` that the blend
reads without the blur having written it makes the result NaN, whatever the allocator happened to leave there.
Bound: max |got - want| < 1e-5 on blocks in [0, 1) (edgetaper_3d_test.m:4,40)."""
import numpy as np
import pytest
import torch

from oracle import rl_oracle as R
from tests import edgetaper_util as U
from tests.rl_util import assert_close

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _taper_raw(dev, bl_t, work_t, psf_t, shape=None, kshape=None, bl_ptr=None, work_ptr=None, psf_ptr=None):
    """mi_edgetaper3d as is: returns the status, does not raise."""
    from ipp_amd import capi
    nz, ny, nx = shape if shape is not None else bl_t.shape
    kz, ky, kx = kshape if kshape is not None else psf_t.shape
    rc = capi.lib().mi_edgetaper3d(dev.index, capi.current_stream_ptr(dev), bl_t.data_ptr() if bl_ptr is None else bl_ptr,
                                   work_t.data_ptr() if work_ptr is None else work_ptr,
                                   psf_t.data_ptr() if psf_ptr is None else psf_ptr, nx, ny, nz, kx, ky, kz)
    torch.cuda.synchronize(dev)
    return rc


def _taper(dev, bl, psf):
    """(result, work) of one call on a NaN-filled work volume, both on the host."""
    from ipp_amd import capi
    t, p = _t(bl, dev), _t(psf, dev)
    work = torch.full_like(t, float("nan"))
    capi.check(_taper_raw(dev, t, work, p))
    return t.cpu().numpy(), work.cpu().numpy()


def _check_poisoned(name, label, got, work):
    """Finite, within the bound of the oracle, and the input's bits wherever the oracle's mask is exactly 1."""
    bl, _, want, m = U.case(name)
    assert got.shape == bl.shape and got.dtype == np.float32
    finite = np.isfinite(got)
    err = float(np.abs(got[finite].astype(np.float64) - want[finite]).max())
    U.report(f"{name} [{label}]: max |got - want| {err:.3g} (bound {U.BOUND:g}), {int((~finite).sum())} non-finite, "
             f"work written on {float(np.isfinite(work).mean()):.3f} of the block, mask < 1 on {float((m < 1).mean()):.3f}")
    assert finite.all(), f"{name} [{label}]: {int((~finite).sum())} voxels read unwritten work, first at {tuple(np.argwhere(~finite)[0])}"
    assert err < U.BOUND
    plateau = m == np.float32(1.0)
    assert np.array_equal(got[plateau].view(np.uint32), bl[plateau].view(np.uint32))


def _check_direct_witness(name, work):
    """The direct route left `work` alone on every skipped tile (the early return ran) and wrote the whole shell."""
    shape, kshape, _ = U.CASES[name]
    m = U.case(name)[3]
    skipped = U.skipped_tiles(shape, kshape)
    assert skipped, name
    for tile in skipped:
        assert np.isnan(work[U.tile_centre(tile)]), f"{name}: tile {tile} was computed"
        (z0, z1), (y0, y1), (x0, x1) = tile
        assert np.isnan(work[z0:z1, y0:y1, x0:x1]).all(), f"{name}: tile {tile} was partly written"
    assert np.isfinite(work[m < 1]).all()


@pytest.mark.parametrize("engine", U.ENGINES)
@pytest.mark.parametrize("name", U.ODD_CASES)
def test_edgetaper_on_poisoned_work(dev, name, engine, monkeypatch):
    """Skipped tiles and rows of more than 256 samples, the 12-sample ramp, plateaus of one sample, extents of 2 and 1, a PSF
    larger than the block: each on all three routes ("slabs" falls back where the slab plan refuses the shape)."""
    monkeypatch.setenv("MI_EDGETAPER_ENGINE", engine)
    bl, psf, _, _ = U.case(name)
    got, work = _taper(dev, bl, psf)
    _check_poisoned(name, engine, got, work)
    if engine == "direct" and name in ("tile_skip_264", "three_strides_600"):
        _check_direct_witness(name, work)


@pytest.mark.parametrize("name", U.EVEN_CASES)
def test_edgetaper_even_psf_extents_take_the_direct_route(dev, name, monkeypatch):
    """An even extent forces the direct route with the reference's window (k / 2 samples before the output, conv3d_gpu.cu:77):
    every setting of the variable gives the same bits, within the bound of the oracle."""
    bl, psf, _, _ = U.case(name)
    results = {}
    for engine in U.ENGINES + (None,):
        if engine is None:
            monkeypatch.delenv("MI_EDGETAPER_ENGINE", raising=False)
        else:
            monkeypatch.setenv("MI_EDGETAPER_ENGINE", engine)
        got, work = _taper(dev, bl, psf)
        _check_poisoned(name, str(engine), got, work)
        if U.CASES[name][0] == (18, 40, 264):
            _check_direct_witness(name, work)   # whatever the variable says, the route is the direct one
        results[engine] = got
    for engine, got in results.items():
        assert np.array_equal(got.view(np.uint32), results["direct"].view(np.uint32)), engine


# ------------------------------------------------------------------ engines kept by a deconvolution plan
_F_XYZ = (64, 64, 32)
_oracle_cache = {}


def _plan_blocks():
    psf = R.gaussian_psf((7, 5, 5), (1.5, 1.0, 1.0))
    a = R.bead_volume((20, 36, 44), seed=21, psf=psf)
    b = np.ascontiguousarray(a[::-1, ::-1])
    half = np.ascontiguousarray(psf * np.float32(0.5))
    small = np.ascontiguousarray(a[:, :32, :40])
    return [("A", a, psf), ("B", b, psf), ("A", a, psf), ("A, PSF x 0.5", a, half), ("smaller block", small, psf), ("A", a, psf)]


def _plan_oracle(label, use_fft, vol, psf):
    key = (label, use_fft)
    if key not in _oracle_cache:
        _oracle_cache[key] = R.decon_fft(vol, psf, _F_XYZ[::-1], 2) if use_fft else R.decon_spatial(vol, psf, 2)
    return _oracle_cache[key]


@pytest.mark.parametrize("use_fft", [True, False])
@pytest.mark.parametrize("engine", ["fft", "slabs"])
def test_plan_keeps_the_taper_engines_bit_identically(dev, engine, use_fft, monkeypatch):
    """TaperKeep::full / TaperKeep::slab[d] serve both sides of an axis and every later block of the same shape and PSF: a
    repeated block, new content, a scaled PSF, a smaller block and the first block again give the bits of the same call without a
    plan (DeconPlan's contract), and the oracle's values."""
    from ipp_amd import decon
    monkeypatch.setenv("MI_EDGETAPER_ENGINE", engine)
    fshape = _F_XYZ if use_fft else None
    with decon.DeconPlan(dev) as plan:
        for step, (label, vol, psf) in enumerate(_plan_blocks()):
            want = decon.decon(_t(vol, dev), psf, 2, 0.0, 0.0, 0, None, use_fft, fshape, False).cpu().numpy()
            got = decon.decon(_t(vol, dev), psf, 2, 0.0, 0.0, 0, None, use_fft, fshape, False, plan=plan).cpu().numpy()
            differ = int((got.view(np.uint32) != want.view(np.uint32)).sum())
            U.report(f"plan [{engine}, use_fft={use_fft}] step {step + 1} ({label}): {differ} voxels differ from the call without a plan")
            assert differ == 0, (step + 1, label)
            assert_close(got, _plan_oracle(label, use_fft, vol, psf), what=f"step {step + 1} ({label})")


# ------------------------------------------------------------------ refusals
def test_edgetaper_refusals_leave_the_block_alone(dev):
    from ipp_amd import capi
    bl = np.random.default_rng(7).random((6, 8, 10), dtype=np.float32)
    t, p = _t(bl, dev), _t(R.gaussian_psf((3, 3, 3), (0.8, 0.8, 0.8)), dev)
    work = torch.full_like(t, float("nan"))

    def refused(message, **kw):
        assert _taper_raw(dev, t, work, p, **kw) == capi.MI_ERR_INVALID
        assert message in capi.last_error(), capi.last_error()
        assert np.array_equal(t.cpu().numpy().view(np.uint32), bl.view(np.uint32))
        assert bool(torch.isnan(work).all())

    refused("edgetaper_3d: null or aliased buffers", work_ptr=t.data_ptr())
    refused("edgetaper_3d: null or aliased buffers", bl_ptr=0)
    refused("edgetaper_3d: null or aliased buffers", work_ptr=0)
    refused("edgetaper_3d: null or aliased buffers", psf_ptr=0)
    refused("edgetaper_3d: bl and psf must be 3D", shape=(6, 8, 0))
    refused("edgetaper_3d: bl and psf must be 3D", shape=(0, 8, 10))
    refused("edgetaper_3d: bl and psf must be 3D", kshape=(3, 0, 3))
    # and the same buffers are taken once nothing is wrong with the call
    capi.check(_taper_raw(dev, t, work, p))
    assert np.abs(t.cpu().numpy() - R.edgetaper_3d(bl, p.cpu().numpy())).max() < U.BOUND
