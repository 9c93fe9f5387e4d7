"""GPU: the TeraFly conversion (ipp_amd.terafly, teraconverter.py) reproduces the reference binary's trees, and mi_pyramid_slab
equals the numpy restatement (tests/terafly_util.py, itself checked against the binary)."""
import ctypes as C
import os
import shlex
import subprocess
import sys

import numpy as np
import pytest
from PIL import Image, ImageSequence

from tests import terafly_util as tu
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu
CLI = os.path.join(ROOT, "image-preprocessing-pipeline_amd", "teraconverter.py")
BASE = ["--sfmt=TIFF (series, 2D)", "--dfmt=TIFF (tiled, 3D)", "--clist=0", "--noprogressbar"]


def _series(vol, folder):
    folder.mkdir()
    for k in range(vol.shape[0]):
        Image.fromarray(vol[k]).save(folder / f"slice_{k:04d}.tif")


def _tree(out):
    return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)


def _pages(path):
    im = Image.open(path)
    return np.stack([np.asarray(p) for p in ImageSequence.Iterator(im)]), int(im.tag_v2.get(259))


def _check_against_golden(g, out):
    assert _tree(out) == [str(f) for f in g["files"]]
    for f in g["files"]:
        f = str(f)
        if f.endswith("mdata.bin"):
            assert (out / f).read_bytes() == g[f"mdata/{f}"].tobytes(), f
            continue
        pages, comp = _pages(out / f)
        n, h, w, gcomp = (int(v) for v in g[f"pages/{f}"])
        assert pages.shape == (n, h, w) and comp == gcomp, f
        if f"sample/{f}" in g.files:
            np.testing.assert_array_equal(pages[g[f"sample_idx/{f}"]], g[f"sample/{f}"], err_msg=f)
        assert tu.pages_sha(pages) == str(g[f"sha/{f}"]), f


@pytest.mark.parametrize("name", tu.golden_runs())
def test_teraconverter_reproduces_golden_tree(name, tmp_path, dev):
    from ipp_amd import teraconverter
    g = tu.load_golden(name)
    src, out = tmp_path / "src", tmp_path / "out"
    _series(tu.golden_input(g), src)
    out.mkdir()
    rc = teraconverter.main(BASE + [str(f) for f in g["flags"]] + [f"-s={src}", f"-d={out}"])
    assert rc == 0
    _check_against_golden(g, out)


def test_slab_rows_do_not_change_the_tree(tmp_path, dev):
    from ipp_amd import teraconverter
    g = tu.load_golden("u16_tiled")
    src = tmp_path / "src"
    _series(tu.golden_input(g), src)
    outs = []
    for rows in (8, 24, 100000):
        out = tmp_path / f"out{rows}"
        out.mkdir()
        assert teraconverter.main(BASE + [str(f) for f in g["flags"]] + [f"-s={src}", f"-d={out}", f"--slab_rows={rows}"]) == 0
        _check_against_golden(g, out)
        outs.append(out)
    for f in _tree(outs[0]):
        assert (outs[0] / f).read_bytes() == (outs[1] / f).read_bytes() == (outs[2] / f).read_bytes(), f


# ------------------------------------------------------------------------------------------------------------------ kernel
def _restated(slab, halve_d, method):
    out, a = [], slab
    for h in halve_d:
        a = tu.halve3d(a, method) if h else tu.halve2d(a, method)
        out.append(a)
    return out


def _run_kernel(slab_t, halve_d, method, want=None):
    import torch
    from ipp_amd import terafly
    shapes = terafly.level_shapes(tuple(slab_t.shape), len(halve_d), halve_d)
    outs = [torch.full(s, 0xAB, dtype=slab_t.dtype, device=slab_t.device) if (want is None or want[k]) else None
            for k, s in enumerate(shapes)]
    terafly.pyramid_slab(slab_t, len(halve_d), halve_d, method, outs)
    torch.cuda.synchronize()
    return [None if o is None else o.cpu().numpy() for o in outs]


CASES = [
    # (nz, ny, nx, halve_d)
    (18, 67, 75, [1, 1, 1]),            # odd extents, the 37-slice group size
    (1, 271, 301, [1, 1, 1]),           # a 1-slice leftover group: every 3-D level empty
    (5, 64, 128, [1, 1, 1, 1]),         # a leftover group, rows a multiple of 4 (vector loads)
    (9, 33, 41, [0, 1, 0, 1, 1]),       # 2-D and 3-D levels mixed
    (4, 40, 36, [0, 0]),                # 2-D only
    (64, 130, 260, [1, 1, 1, 1, 1, 1]), # six levels: three chained launches
    (7, 9, 10, [1]),                    # one level: a launch without a second level
]


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("method", ["mean", "max"])
@pytest.mark.parametrize("case", range(len(CASES)))
def test_pyramid_slab_equals_restatement(dev, dtype, method, case):
    import torch
    nz, ny, nx, hd = CASES[case]
    rng = np.random.default_rng(100 + case)
    slab = rng.integers(0, np.iinfo(dtype).max + 1, (nz, ny, nx), dtype=dtype)
    got = _run_kernel(torch.from_numpy(slab).to(dev), hd, method)
    for k, want in enumerate(_restated(slab, hd, method)):
        assert got[k].shape == want.shape, (k, got[k].shape, want.shape)
        np.testing.assert_array_equal(got[k], want, err_msg=f"level {k + 1}")


def test_pyramid_slab_skips_unwanted_levels(dev):
    import torch
    rng = np.random.default_rng(7)
    slab = rng.integers(0, 65536, (16, 70, 90), dtype=np.uint16)
    hd = [1, 1, 1, 1]
    got = _run_kernel(torch.from_numpy(slab).to(dev), hd, "mean", want=[False, True, False, True])
    want = _restated(slab, hd, "mean")
    assert got[0] is None and got[2] is None
    np.testing.assert_array_equal(got[1], want[1])
    np.testing.assert_array_equal(got[3], want[3])


def test_pyramid_slab_refuses_a_missing_chain_buffer(dev):
    import torch
    from ipp_amd import capi, terafly
    slab = torch.zeros((8, 16, 16), dtype=torch.uint16, device=dev)
    with pytest.raises(capi.MiError, match="feeds level 3"):
        terafly.pyramid_slab(slab, 3, [1, 1, 1], "mean", [None, None, torch.zeros((1, 2, 2), dtype=torch.uint16, device=dev)])


def test_pyramid_slab_past_2_31_samples(dev):
    """A slab of 2 slices whose planes together pass 2^31 samples: the last rows (beyond the 32-bit range) equal the
    restatement."""
    import torch
    nz, ny, nx = 2, 32768 + 6, 32768 + 2
    assert nz * ny * nx > 2 ** 31
    g = torch.Generator(device=dev)
    g.manual_seed(11)
    slab = torch.randint(0, 256, (nz, ny, nx), dtype=torch.uint8, device=dev, generator=g)
    got = _run_kernel(slab, [1, 1], "mean")
    tail = slab[:, ny - 256:, :].cpu().numpy()          # rows ny-256.. -> level-1 rows (ny-256)/2.., level-2 rows (ny-256)/4..
    want = _restated(tail, [1, 1], "mean")
    np.testing.assert_array_equal(got[0][:, (ny - 256) // 2:], want[0])
    np.testing.assert_array_equal(got[1][:, (ny - 256) // 4:], want[1])
    del slab
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ pipeline
def _pipeline_command(src, dst):
    """The pipeline's TeraFly command line (process_images.py), with this converter in place of the binary."""
    return " ".join([shlex.quote(sys.executable), shlex.quote(CLI), "--sfmt=\"TIFF (series, 2D)\"", "--dfmt=\"TIFF (tiled, 3D)\"",
                     "--resolutions=\"012345\"", "--clist=0", "--halve=mean", "-s=" + shlex.quote(str(src)),
                     "-d=" + shlex.quote(str(dst))])


def _run_pipeline_command(src, dst, vol):
    dst.mkdir()
    p = subprocess.run(_pipeline_command(src, dst), shell=True, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    files, mdata = tu.convert(vol, ["--resolutions=012345"])
    assert _tree(dst) == sorted(list(files) + [f"{r}/mdata.bin" for r in mdata])
    for f, want in files.items():
        np.testing.assert_array_equal(_pages(dst / f)[0], want, err_msg=f)
    for r, b in mdata.items():
        assert (dst / r / "mdata.bin").read_bytes() == b


def test_pipeline_command_on_a_step6_tree(tmp_path, dev):
    """-6 with the default slice size writes one tile folder of deflated 2-D slices (the device TIFF writer): a 2-D series."""
    import torch
    from ipp_amd import brickio
    rng = np.random.default_rng(21)
    vol = rng.integers(0, 65536, (66, 257, 263), dtype=np.uint16)
    src = tmp_path / "RES(257x263x66)" / "000000" / "000000_000000"
    src.mkdir(parents=True)
    brickio.save_tiff_series_device(src, torch.from_numpy(vol).to(dev))
    _run_pipeline_command(src, tmp_path / "terafly", vol)


def test_pipeline_command_on_a_decwrap_folder(tmp_path, dev):
    from ipp_amd import brickio
    rng = np.random.default_rng(22)
    vol = rng.integers(0, 256, (65, 251, 259), dtype=np.uint8)
    src = tmp_path / "deconvolved"
    src.mkdir()
    brickio.save_tiff_series(src, vol)
    _run_pipeline_command(src, tmp_path / "terafly", vol)
