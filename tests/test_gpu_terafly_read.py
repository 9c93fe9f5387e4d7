"""GPU: the device reader of TeraFly trees (mi_tiff3d_read_box_device: k_strip_lzw, k_tree_place; TeraFlyTree.imread_device;
teraextract.py).  The yardsticks are the host reader on the same files (mi_tiff3d_read_box, itself checked against the numpy
restatement, Pillow and an independent Python decoder by tests/test_terafly_read_host.py and tests/test_tiff_lzw_host.py), and
mi_pyramid_slab's planes for a tree the device wrote; everything is exact.

The kernel runs the decoder text of csrc/tiff_lzw_dev.h; tests/test_tiff_lzw_host.py proves that text on the same corpus and the same
malformed list under the host sanitizers and is the precondition of the refusal test here."""
import ctypes as C
import glob
import os

import numpy as np
import pytest
import torch

from ipp_amd import brickio, capi, terafly
from tests import lzw_util as lu
from tests import terafly_read_util as ru

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN_READ = os.path.join(ROOT, "tests", "golden", "terafly_read")


def _jobs(items):
    """items: [(path, pages, rows, cols, oz)] whole files"""
    return (capi.Tiff3dJob * len(items))(*[capi.Tiff3dJob(os.fsencode(p), 0, n, 0, h, 0, w, oz, 0, 0) for p, n, h, w, oz in items])


def _read_both(items, box, dev):
    """the box of uint8 through both readers: (host bytes, device bytes, host error, device error)"""
    jobs = _jobs(items)
    lib = capi.lib()
    host = np.full(box, 0xee, np.uint8)
    rc_h = lib.mi_tiff3d_read_box(jobs, len(items), box[0], box[1], box[2], 1, host.ctypes.data, 2)
    err_h = capi.last_error() if rc_h else None
    out = torch.full(box, 0xee, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc_d = lib.mi_tiff3d_read_box_device(dev.index, capi.current_stream_ptr(dev), jobs, len(items), box[0], box[1], box[2], 1, out.data_ptr(), 2)
    err_d = capi.last_error() if rc_d else None
    return host, out.cpu().numpy(), err_h, err_d


def test_every_corpus_stream_as_the_strip_of_a_one_page_file(dev, tmp_path):
    """(but the empty strip: a page has at least a byte)"""
    seen = 0
    for name, (stream, data) in sorted(lu.corpus().items()):
        if not data:
            continue
        f = ru.strip_tiff(tmp_path / f"{name}.tif", stream, len(data))
        host, got, eh, ed = _read_both([(f, 1, 1, len(data), 0)], (1, 1, len(data)), dev)
        assert eh is None and ed is None, (name, eh, ed)
        assert got.tobytes() == host.tobytes() == data, name
        seen += 1
    assert seen == 11


def test_every_malformed_stream_ends_with_its_status_and_message(dev, tmp_path):
    """the streams tests/test_tiff_lzw_host.py has passed through the same decoder text under the sanitizers: each is refused with
    the host reader's words"""
    for name, stream, size, want in lu.malformed():
        f = ru.strip_tiff(tmp_path / f"{name}.tif", stream, size)
        _, _, eh, ed = _read_both([(f, 1, 1, size, 0)], (1, 1, size), dev)
        assert eh is not None and eh == ed, (name, eh, ed)
        assert f"{name}.tif: page 0: strip 0 does not decode to its rows (status {want}: {lu.STATUS_NAMES[want]})" in ed, (name, ed)


def test_strips_of_1_byte_512_bytes_and_64_kb_in_one_launch(dev, tmp_path):
    """the three table sizes of a call and the strings longer than a wave in one batch; a 70 000-byte strip takes the 32-bit offsets"""
    rng = np.random.default_rng(9)
    datas = [b"\x42", (np.arange(512) // 7 % 251).astype(np.uint8).tobytes(), b"\xc3" * 65536,
             np.repeat(rng.integers(0, 256, 700, dtype=np.uint8), 100).tobytes(), rng.integers(0, 256, 16384, dtype=np.uint8).tobytes(),
             np.repeat(rng.integers(0, 4, 1639, dtype=np.uint8), 10)[:16385].tobytes()]
    items = [(ru.strip_tiff(tmp_path / f"s{k}.tif", lu.encode(d), len(d)), 1, 1, len(d), k) for k, d in enumerate(datas)]
    host, got, eh, ed = _read_both(items, (len(datas), 1, 70000), dev)
    assert eh is None and ed is None, (eh, ed)
    assert got.tobytes() == host.tobytes()
    for k, d in enumerate(datas):
        assert got[k, 0, :len(d)].tobytes() == d and (got[k, 0, len(d):] == 0xee).all(), k


@pytest.fixture(scope="module")
def trees(tmp_path_factory):
    out = {}
    for name in ru.TREES:
        root = str(tmp_path_factory.mktemp(name))
        out[name] = (root, ru.write_tree(root, name))
    return out


@pytest.mark.parametrize("name", sorted(ru.TREES))
def test_imread_device_equals_imread_by_both_routes(dev, trees, name):
    root, levels = trees[name]
    t = terafly.open_tree(root)
    for k, (lv, want) in enumerate(zip(t.levels, levels)):
        for box in ru.boxes(lv.shape, ru.seams_of(lv)):
            z0, z1, y0, y1, x0, x1 = box
            host = t.imread(box, k)
            assert host.tobytes() == want[z0:z1, y0:y1, x0:x1].tobytes()
            for route in ("device", "host"):
                got = t.imread_device(box, k, device=dev, route=route)
                assert got.device == dev and tuple(got.shape) == host.shape
                got = got.cpu().numpy()
                assert got.dtype == host.dtype and got.tobytes() == host.tobytes(), (name, k, box, route)


def test_the_route_switch_is_read_per_call(dev, trees, monkeypatch):
    root, levels = trees["u16_lzw_rps1_tiled"]
    t = terafly.open_tree(root)
    box = (1, 3, 240, 260, 245, 262)
    for value in ("1", "0", None):
        if value is None:
            monkeypatch.delenv("MI_TERAFLY_READ_DEVICE", raising=False)
        else:
            monkeypatch.setenv("MI_TERAFLY_READ_DEVICE", value)
        assert t.imread_device(box, device=dev).cpu().numpy().tobytes() == levels[0][1:3, 240:260, 245:262].tobytes()
    with pytest.raises(ValueError, match="route"):
        t.imread_device(box, device=dev, route="gpu")


def test_the_golden_trees(dev):
    from PIL import Image, ImageSequence
    for run in ("planes_u8", "ramp_u16", "sparse_u16"):
        t = terafly.open_tree(os.path.join(GOLDEN_READ, run))
        for k, lv in enumerate(t.levels):
            f, = glob.glob(os.path.join(str(lv.path), "*", "*", "*.tif"))
            pages = np.stack([np.asarray(p) for p in ImageSequence.Iterator(Image.open(f))])
            got = t.imread_device((0, lv.shape[0], 0, lv.shape[1], 0, lv.shape[2]), k, device=dev, route="device").cpu().numpy()
            assert got.dtype == pages.dtype and got.tobytes() == pages.tobytes(), (run, k)
            got = t.imread_device((1, 3, 7, 20, 3, 100), k, device=dev, route="device").cpu().numpy()
            assert got.tobytes() == pages[1:3, 7:20, 3:100].tobytes(), (run, k)


@pytest.fixture(scope="module")
def converted(tmp_path_factory):
    """a series of (37, 271, 301) uint16, its tree written by terafly.convert on the device"""
    vol = ru.volume("uint16", (37, 271, 301), 77)
    src, dst = tmp_path_factory.mktemp("series"), tmp_path_factory.mktemp("tree")
    brickio.save_tiff_series(src, vol, first_index=0)
    p = terafly.convert(str(src), str(dst), resolutions="0123")
    return vol, str(src), str(dst), p


def test_a_tree_written_on_the_device_reads_back_as_the_pyramids_planes(dev, converted):
    vol, src, dst, p = converted
    halve_d = [1, 1, 1]
    want = [[], [], [], []]
    for z, n in p.groups():
        slab = torch.from_numpy(vol[z:z + n]).to(dev)
        outs = [torch.empty(s, dtype=torch.uint16, device=dev) for s in terafly.level_shapes(slab.shape, 3, halve_d)]
        terafly.pyramid_slab(slab, 3, halve_d, "mean", outs)
        want[0].append(vol[z:z + n])
        for k, o in enumerate(outs):
            want[k + 1].append(o.cpu().numpy())
    t = terafly.open_tree(dst)
    assert [lv.shape for lv in t.levels] == [(37, 271, 301), (18, 135, 150), (8, 67, 75), (4, 33, 37)]
    assert [lv.nominal_depth for lv in t.levels] == [37, 18, 9, 4]
    for k, lv in enumerate(t.levels):
        planes = np.concatenate(want[k], axis=0)
        got = t.imread_device((0, lv.shape[0], 0, lv.shape[1], 0, lv.shape[2]), k, device=dev, route="device").cpu().numpy()
        assert got.shape == planes.shape and got.tobytes() == planes.tobytes(), k


def test_teraextract_writes_the_sub_volume_of_the_source_series(dev, converted, tmp_path):
    from ipp_amd import teraextract
    vol, src, dst, p = converted
    for route, slab in (("device", 4), (None, None)):
        out = tmp_path / f"out_{route}"
        made, box = teraextract.extract(dst, str(out), 0, (10, 200, 33, -1, 5, 16), route=route, slab=slab)
        assert made == 11 and box == (5, 16, 10, 200, 33, 301)
        names = sorted(os.listdir(out))
        assert names == [f"img_{z:06d}.tif" for z in range(5, 16)]
        got = brickio.load_tiff_series(str(out))
        assert got.dtype == vol.dtype and got.tobytes() == vol[5:16, 10:200, 33:301].tobytes()
    assert teraextract.main([f"--src={dst}", f"--dst={tmp_path / 'lv2'}", "--level=2", "--D1=3"]) == 0
    lv2 = terafly.open_tree(dst).imread((0, 3, 0, 67, 0, 75), 2)
    assert brickio.load_tiff_series(str(tmp_path / "lv2")).tobytes() == lv2.tobytes()
    assert teraextract.main([f"--src={dst}", f"--dst={tmp_path / 'no'}", "--level=7"]) == 2
    assert teraextract.main([f"--src={dst}", f"--dst={tmp_path / 'no'}", "--V1=999"]) == 2


def test_scratch_is_kept_grows_and_is_given_back(dev, trees):
    root, levels = trees["u16_lzw_rps1_tiled"]
    t = terafly.open_tree(root)
    small, large = (0, 1, 0, 9, 0, 9), (0,) + (levels[0].shape[0], 0, levels[0].shape[1], 0, levels[0].shape[2])

    def read(box):
        z0, z1, y0, y1, x0, x1 = box
        got = t.imread_device(box, device=dev, route="device").cpu().numpy()
        assert got.tobytes() == levels[0][z0:z1, y0:y1, x0:x1].tobytes()

    capi.release_cached_memory(dev.index)
    read(small)
    read(large)
    read(small)
    assert capi.release_cached_memory(dev.index) >= levels[0].nbytes // 2     # the decoded rows of the large box were scratch
    read(small)
    read(large)
