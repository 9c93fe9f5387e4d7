"""Shared by the stitching-import tests: the cases of tests/golden/stitch_import/ (written by tests/golden/make_import_golden.py
from the reference's own ``terastitcher -1``), their tile folders rebuilt from cases.json, and the element-wise XML comparison."""
import json
import os
import xml.etree.ElementTree as ET

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stitch_import")
AXES = {"V": 1, "H": 2, "D": 3, "1": 1, "2": 2, "3": 3}


def load_cases():
    with open(os.path.join(GOLD, "cases.json")) as f:
        return json.load(f)


def ref_codes(case):
    """The signed axis codes of a case's --ref1..3 strings."""
    return [-AXES[r[1:]] if r.startswith("-") else AXES[r] for r in case["ref"]]


def write_folder(root, case):
    """The folder the golden run read: ``.tif`` names are TIFFs of the case's size and sample format (headers are all the
    import reads), other files hold a few arbitrary bytes -- a stale ``mdata.bin`` among them."""
    from PIL import Image
    h, w = case["tile"]
    img = Image.new("RGB" if case["chans"] == 3 else ("I;16" if case["bits"] == 16 else "L"), (w, h))

    def put(path, name):
        if name.endswith(".tif"):
            img.save(os.path.join(path, name))
        else:
            with open(os.path.join(path, name), "wb") as f:
                f.write(b"\x07stale\x00")

    os.makedirs(root)
    for n1, lev2 in case["tree"].items():
        if lev2 is None:
            put(root, n1)
            continue
        os.makedirs(os.path.join(root, n1))
        for n2, files in lev2.items():
            if files is None:
                put(os.path.join(root, n1), n2)
                continue
            os.makedirs(os.path.join(root, n1, n2))
            for f in files:
                put(os.path.join(root, n1, n2), f)


def write_hvd_tiff_tree(root, npz):
    """The TIFF tree of the chain_hvd golden run: <H>/<H>_<V>/<H>_<V>_<D>.tif, positions in 0.1 um -- the tiles of
    test_gpu_terastitcher_golden.write_tiff_tree with the H coordinate as the first level."""
    from PIL import Image
    rows, cols = int(npz["rows"]), int(npz["cols"])
    vxl = npz["vxl"]
    ov_v, ov_h = (int(v) for v in npz["overlap"])
    for r in range(rows):
        for c in range(cols):
            vol = npz[f"tile_{r}_{c}"]
            step_v, step_h = vol.shape[1] - ov_v, vol.shape[2] - ov_h
            v = int(round(r * step_v * vxl[0] * 10))
            h = int(round(c * step_h * vxl[1] * 10))
            d = os.path.join(root, f"{h:06d}", f"{h:06d}_{v:06d}")
            os.makedirs(d, exist_ok=True)
            for z in range(vol.shape[0]):
                Image.fromarray(vol[z]).save(os.path.join(d, f"{h:06d}_{v:06d}_{int(round(z * vxl[2] * 10)):06d}.tif"))


def golden_text(path, tiles_dir):
    with open(path) as f:
        return f.read().replace("TILES_DIR", str(tiles_dir))


def assert_same_xml(got_path, want_text, what):
    """Element by element, in document order: same tags, same attributes in the same order, every value string-equal."""
    got, want = ET.parse(got_path).getroot(), ET.fromstring(want_text)
    g, w = list(got.iter()), list(want.iter())
    assert [e.tag for e in g] == [e.tag for e in w], what
    for a, b in zip(g, w):
        assert list(a.attrib.items()) == list(b.attrib.items()), (what, a.tag, a.attrib, b.attrib)
        assert [c.tag for c in a] == [c.tag for c in b], (what, a.tag)
