"""GPU: the device TIFF reader (mi_tiff_read_box_device: k_strip_inflate, k_strip_unpredict_crop; brickio.read_tiff_box_device,
load_tiff_series_device; the MI_TIFF_READ_DEVICE switch of TSVVolume.imread_device).  The yardsticks are ``zlib.decompress`` and
the host reader ``read_tiff_box`` on the same files; everything is exact.

The kernel runs the decoder text of csrc/tiff_inflate_dev.h; tests/test_tiff_inflate_host.py proves that text on the same corpus
and the same malformed list under the host sanitizers and is the precondition of the refusal test here."""
import zlib

import numpy as np
import pytest
import torch

from ipp_amd import brickio, capi
from tests import deflate_util as du
from tests import inflate_util as iu
from tests import tsv_util as T

pytestmark = pytest.mark.gpu


def _host(t):
    return t.cpu().numpy()


def _both(files, shape, dtype, box, dev):
    """the box through the device reader, required to equal the host reader's; returns it as numpy"""
    y0, y1, x0, x1 = box
    want = brickio.read_tiff_box(files, shape, dtype, y0, y1, x0, x1)
    got = brickio.read_tiff_box_device(files, shape, dtype, y0, y1, x0, x1, device=dev)
    assert got.device == dev and tuple(got.shape) == want.shape
    got = _host(got)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (shape, str(np.dtype(dtype)), box)
    return got


def test_every_corpus_stream_as_the_strip_of_a_file(dev, tmp_path):
    for name, (stream, data) in sorted(iu.corpus().items()):
        f = iu.stream_tiff(tmp_path / f"{name}.tif", stream + (b"\0\0\0" if name == "runs" else b""), len(data))
        got = _both([f], (1, len(data)), np.uint8, (0, 1, 0, len(data)), dev)
        assert got.tobytes() == zlib.decompress(stream) == data, name


def _image(dtype, seed):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:96, 0:80]
    if np.dtype(dtype) == np.float32:
        return (rng.standard_normal((96, 80)) * 100).astype(np.float32)
    top = 250 if np.dtype(dtype) == np.uint8 else 60000
    a = (top / 2 + top / 3 * np.sin(x / 9.0 + seed) * np.cos(y / 13.0) + rng.integers(0, 6, (96, 80))).astype(dtype)
    a[:, 50:70] = 0                    # runs, and differences that wrap
    a[40:44, :] = top
    return a


BOXES = [(0, 96, 0, 80),      # the full image
         (8, 13, 3, 70),      # inside one strip (of 7, 64 or 96 rows)
         (5, 23, 11, 57),     # across two boundaries of 7-row strips, odd x0 / x1
         (91, 96, 0, 80)]     # the last, partial strip


@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
@pytest.mark.parametrize("compression,predictor", [(8, 1), (8, 2), (32946, 1), (32946, 2)])
def test_boxes_of_integer_files(dev, tmp_path, dtype, compression, predictor):
    for rps in (1, 7, 64, 96):
        imgs = [_image(dtype, 3 * rps + k) for k in range(3)]
        files = [iu.image_tiff(tmp_path / f"r{rps}_{k}.tif", im, rps, compression, predictor) for k, im in enumerate(imgs)]
        for box in BOXES:
            got = _both(files, (96, 80), dtype, box, dev)
            y0, y1, x0, x1 = box
            assert got.tobytes() == np.stack(imgs)[:, y0:y1, x0:x1].tobytes(), (rps, box)


def test_boxes_of_float_files_and_of_raw_strips_longer_than_their_rows(dev, tmp_path):
    for rps in (7, 96):
        imgs = [_image(np.float32, 50 + k) for k in range(3)]
        files = [iu.image_tiff(tmp_path / f"f{rps}_{k}.tif", im, rps, 8, 1) for k, im in enumerate(imgs)]
        for box in BOXES:
            got = _both(files, (96, 80), np.float32, box, dev)
            assert got.tobytes() == np.stack(imgs)[:, box[0]:box[1], box[2]:box[3]].tobytes()
    for dtype, predictor in ((np.uint8, 1), (np.uint16, 2), (np.float32, 1)):
        for rps in (7, 64):
            imgs = [_image(dtype, 70 + k) for k in range(3)]
            files = [iu.image_tiff(tmp_path / f"raw{np.dtype(dtype).name}{rps}_{k}.tif", im, rps, 1, predictor, pad=5 + 2 * k) for k, im in enumerate(imgs)]
            for box in BOXES:
                got = _both(files, (96, 80), dtype, box, dev)
                assert got.tobytes() == np.stack(imgs)[:, box[0]:box[1], box[2]:box[3]].tobytes()


def _round_trip_volumes():
    disc = du.sparse_disc(np.uint16)
    sparse = np.stack([np.roll(disc, 7 * z, axis=1) for z in range(64)])
    rng = np.random.default_rng(12)
    base = (np.cumsum(rng.standard_normal((4, 1024, 1024)), axis=2) * 6 + 3000 + rng.random((4, 1024, 1024)) * 40).clip(0, 65535).astype(np.uint16)
    smooth = np.stack([np.roll(base[z % 4], 13 * z, axis=0) for z in range(64)])
    return [("sparse", sparse), ("smooth", smooth)]


def test_round_trip_of_the_device_writer(dev, tmp_path):
    for name, vol in _round_trip_volumes():
        t = torch.from_numpy(vol).to(dev)
        assert brickio.save_tiff_series_device(tmp_path / name, t) == 64
        files = brickio.list_tiff_series(tmp_path / name)
        assert len(files) == 64 and all(du.file_strips(f)[2] < 1024 for f in files[:2])      # several strips per slice
        back = brickio.read_tiff_box_device(files, (1024, 1024), np.uint16, 0, 1024, 0, 1024, device=dev)
        assert back.dtype == torch.uint16 and tuple(back.shape) == (64, 1024, 1024)
        assert torch.equal(back.view(torch.int16), t.view(torch.int16)), name
        part = brickio.read_tiff_box_device(files[10:13], (1024, 1024), np.uint16, 500, 530, 7, 1001, device=dev)   # across the strips' boundary
        assert torch.equal(part.view(torch.int16), t[10:13, 500:530, 7:1001].view(torch.int16)), name
        whole = brickio.load_tiff_series_device(tmp_path / name, device=dev)
        assert torch.equal(whole.view(torch.int16), t.view(torch.int16)), name
        z = brickio.load_tiff_series_device(tmp_path / name, 3, 5, device=dev)
        assert torch.equal(z.view(torch.int16), t[3:5].view(torch.int16))


def test_refusals_name_the_file_and_the_strip(dev, tmp_path):
    good_stream, good = iu.corpus()["img"]
    good_file = iu.stream_tiff(tmp_path / "good.tif", good_stream, len(good))
    for name, stream, size, status in iu.malformed():
        f = iu.stream_tiff(tmp_path / f"{name}.tif", stream, size)
        with pytest.raises(capi.MiError) as e:
            brickio.read_tiff_box_device([f], (1, size), np.uint8, 0, 1, 0, size, device=dev)
        assert e.value.code == capi.MI_ERR_INVALID
        assert f"{name}.tif" in str(e.value) and "strip 0" in str(e.value) and iu.STATUS_NAMES[status] in str(e.value), str(e.value)
    got = brickio.read_tiff_box_device([good_file], (1, len(good)), np.uint8, 0, 1, 0, len(good), device=dev)
    assert _host(got).tobytes() == good


def test_load_tiff_series_device_does_not_read_a_refused_series_on_the_host(dev, tmp_path):
    """a first file that IS fast: what the device reader refuses is the caller's error, never a quiet host read"""
    stream, img = iu.corpus()["img"]
    iu.stream_tiff(tmp_path / "img_000000.tif", stream, len(img))
    flipped = bytearray(stream)
    flipped[len(stream) // 3] ^= 0x55
    iu.stream_tiff(tmp_path / "img_000001.tif", bytes(flipped), len(img))
    with pytest.raises(capi.MiError) as e:
        brickio.load_tiff_series_device(tmp_path, device=dev)
    assert e.value.code == capi.MI_ERR_INVALID and "img_000001.tif" in str(e.value) and "strip 0" in str(e.value)
    got = brickio.load_tiff_series_device(tmp_path, 0, 1, device=dev)
    assert _host(got).tobytes() == img
    iu.image_tiff(tmp_path / "img_000002.tif", _image(np.uint8, 1), 7)
    with pytest.raises(ValueError, match="differs from the first slice"):
        brickio.load_tiff_series_device(tmp_path, 0, 3, device=dev)


def _message(fn):
    with pytest.raises(capi.MiError) as e:
        fn()
    assert e.value.code == capi.MI_ERR_INVALID
    return str(e.value)


def test_files_the_host_reader_refuses_are_refused_in_its_words(dev, tmp_path):
    from PIL import Image
    img = _image(np.uint16, 1)
    lzw = tmp_path / "lzw.tif"
    Image.fromarray(img).save(lzw, format="TIFF", compression="tiff_lzw")
    ok = iu.image_tiff(tmp_path / "ok.tif", img, 7)
    other = iu.image_tiff(tmp_path / "other.tif", img[:, :64], 7)
    for files in ([lzw], [ok, other]):
        host = _message(lambda: brickio.read_tiff_box(files, (96, 80), np.uint16, 0, 96, 0, 80))
        device = _message(lambda: brickio.read_tiff_box_device(files, (96, 80), np.uint16, 0, 96, 0, 80, device=dev))
        assert device == host
    assert "not a file this reader decodes" in _message(lambda: brickio.read_tiff_box_device([lzw], (96, 80), np.uint16, 0, 96, 0, 80, device=dev))
    assert "differs from the first slice" in _message(lambda: brickio.read_tiff_box_device([ok, other], (96, 80), np.uint16, 0, 96, 0, 80, device=dev))
    # strips the directory misplaces: the same checks, so the same words
    raw = img.tobytes()
    outside = iu.make_tiff(tmp_path / "outside.tif", [zlib.compress(raw, 1)], 80, 96, 16, 96, 8, counts=[1 << 20])
    rows7 = [raw[r * 7 * 160:(r + 1) * 7 * 160] for r in range(14)]
    rows7[1] = rows7[1][:100]
    short = iu.make_tiff(tmp_path / "short.tif", rows7, 80, 96, 16, 7, 1)
    for f, words, box in ((outside, "a strip lies outside the file", (0, 96)), (short, "strip shorter than its rows", (3, 20))):
        host = _message(lambda: brickio.read_tiff_box([f], (96, 80), np.uint16, box[0], box[1], 0, 80))
        device = _message(lambda: brickio.read_tiff_box_device([f], (96, 80), np.uint16, box[0], box[1], 0, 80, device=dev))
        assert device == host and words in host
    # load_tiff_series_device: a first file that is not fast is read on the host and uploaded
    folder = tmp_path / "series"
    folder.mkdir()
    for k in range(2):
        Image.fromarray(_image(np.uint16, 20 + k)).save(folder / f"img_{k:06}.tif", format="TIFF", compression="tiff_lzw")
    got = brickio.load_tiff_series_device(folder, device=dev)
    assert got.device == dev and _host(got).tobytes() == brickio.load_tiff_series(folder).tobytes()


def test_the_switch_of_tsvvolume_changes_no_sample(dev, tmp_path, monkeypatch):
    from ipp_amd import tsv
    case = T.Case("inflate_switch", np.uint16, 2, 2, 64, 64, 4, 20, seed=31, max_d=1)
    xml = case.write(tmp_path, lambda path, plane: iu.image_tiff(path, plane, 24, 8, 2))
    calls = []
    real = brickio.read_tiff_box_device
    monkeypatch.setattr(brickio, "read_tiff_box_device", lambda *a, **k: calls.append(1) or real(*a, **k))
    boxes = {}
    for switch in (None, "1"):
        if switch is None:
            monkeypatch.delenv("MI_TIFF_READ_DEVICE", raising=False)
        else:
            monkeypatch.setenv("MI_TIFF_READ_DEVICE", switch)
        v = tsv.TSVVolume(xml, cosine_blending=True, device=dev)
        e = v.volume
        sub = tsv.VExtent(e.x0 + 9, e.x1 - 5, e.y0 + 3, e.y1 - 11, e.z0 + 1, e.z1)
        boxes[switch] = [_host(v.imread_device(b)) for b in (e, sub)]
        assert bool(calls) == (switch == "1")
    for a, b in zip(boxes[None], boxes["1"]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def test_scratch_is_kept_grows_and_is_given_back(dev, tmp_path):
    small = [iu.image_tiff(tmp_path / "s.tif", _image(np.uint16, 5), 7, 8, 2)]
    imgs = [np.random.default_rng(k).integers(0, 4000, (700, 900)).astype(np.uint16) for k in range(3)]
    large = [iu.image_tiff(tmp_path / f"l{k}.tif", im, 64, 8, 1) for k, im in enumerate(imgs)]
    _both(small, (96, 80), np.uint16, (0, 96, 0, 80), dev)
    got = _both(large, (700, 900), np.uint16, (1, 699, 1, 899), dev)
    assert got.tobytes() == np.stack(imgs)[:, 1:699, 1:899].tobytes()
    capi.release_cached_memory(dev.index)
    _both(small, (96, 80), np.uint16, (5, 23, 11, 57), dev)
    _both(large, (700, 900), np.uint16, (0, 700, 0, 900), dev)
