#!/usr/bin/env python3
"""Golden fixtures of the TSVVolume merge from the reference's OWN ``tsv.volume.TSVVolume(...).imread`` (build container only: it
reads the reference tree through ``tests/tsv_util.import_reference``: the stand-ins of tests/pystripe_util.py for what
``pystripe.core`` imports, ``tifffile.imread`` replaced by this project's TIFF reader, and ``USE_NUMEXPR = False`` -- numexpr is
not installed, so the reference's numpy branch is what the goldens hold).

For every case of tests/tsv_util.CASES the tiles are written from their seeds to a temporary folder, the reference reads the whole
extent with ``cosine_blending`` False and True, and tests/golden/tsv/ receives

    <case>.xml      the project XML the reference read, its stacks_dir replaced by the placeholder TILES_DIR
    <case>.npz      x0 / y0 / z0 [rows, cols] (the reference's offsets), extent [6] = x0 x1 y0 y1 z0 z1, and the volumes ``max`` and
                    ``cosine`` (only the blends the case lists)

The numpy restatement (tests/tsv_util.merge_restatement) must equal the reference exactly on every case, sub-boxes included, or
nothing is written.
"""
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import tsv_util as T  # noqa: E402


def main():
    from ipp_amd import pystripe
    imsave = lambda path, plane: pystripe.imsave_tif(path, plane, None)  # noqa: E731
    tv = T.import_reference("/root/reference", lambda path: pystripe.imread_tif_raw_png(path))
    T.GOLDEN_DIR.mkdir(parents=True, exist_ok=True)
    total = 0
    for case in T.CASES.values():
        with tempfile.TemporaryDirectory() as tmp:
            xml = case.write(tmp, imsave)
            stacks, x0, y0, z0, extent = T.case_stacks(case)
            fields = {}
            for blend in case.blends:
                vol = tv.TSVVolume(str(xml), ignore_z_offsets=case.ignore_z_offsets, cosine_blending=blend == "cosine")
                assert vol.dtype == case.dtype.type, (case.name, vol.dtype)
                ext = vol.volume
                got = (ext.x0, ext.x1, ext.y0, ext.y1, ext.z0, ext.z1)
                assert got == extent, (case.name, got, extent)
                offs = np.array([[(o.x, o.y, o.z) for o in row] for row in vol.offsets])
                assert np.array_equal(offs[..., 0].reshape(-1), x0) and np.array_equal(offs[..., 1].reshape(-1), y0) and \
                    np.array_equal(offs[..., 2].reshape(-1), z0), case.name
                with np.errstate(all="ignore"):
                    full = vol.imread(ext, vol.dtype)
                assert full.dtype == case.dtype and full.shape == ext.shape
                mine = T.merge_restatement(stacks, x0, y0, z0, extent, blend == "cosine")
                assert np.array_equal(mine, full), (case.name, blend, int((mine != full).sum()))
                # sub-boxes: the reference's result of a box is the same slice of its full read, and the restatement's too
                for box in T.sub_boxes(extent):
                    with np.errstate(all="ignore"):
                        part = vol.imread(tv.VExtent(*box), vol.dtype)
                    assert np.array_equal(part, T.slice_of(full, extent, box)), (case.name, blend, box)
                    assert np.array_equal(T.merge_restatement(stacks, x0, y0, z0, box, blend == "cosine"), part), (case.name, blend, box)
                fields[blend] = full
                fields.update(x0=offs[..., 0].astype(np.int32), y0=offs[..., 1].astype(np.int32), z0=offs[..., 2].astype(np.int32),
                              extent=np.array(got, np.int32))
            (T.GOLDEN_DIR / f"{case.name}.xml").write_text(case.xml())
            path = case.golden_path()
            np.savez_compressed(path, **fields)
            size = os.path.getsize(path)
            assert size < 1 << 20, (case.name, size)
            total += size
            print(f"{case.name:12s} extent {extent} blends {','.join(case.blends)}: restatement == reference, {size / 1024:.0f} KiB")
    print(f"total {total / 1e3:.0f} kB in {len(T.CASES)} cases")


if __name__ == "__main__":
    main()
