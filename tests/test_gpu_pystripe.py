"""GPU: the pystripe stage (ipp_amd.pystripe, include/mi_pystripe.h) against the goldens of the reference's own code and the
float64 restatement of tests/pystripe_util.py.  Reads tests/golden/ and tests/pystripe_util.py only.

Standards (from the reference, not from the code under test):
  * log domain: max |device - float64 restatement| <= 4 E_ref, E_ref = the float32 reference's own distance from the same float64
    result (stored per golden);
  * integer results: every pixel within 1 + ceil(5 E_ref (v + 1)) counts of the golden's value v, at most 1 % of the pixels differ;
  * float results: |device - golden| <= 5 E_ref (|v| + 1) (the same propagation through expm1, no rounding count).
Every measured figure is printed before it is asserted; PYSTRIPE_REPORT=<file> appends them to a file (profiles/r08_pystripe.txt was
collected that way).
"""
import ctypes as C
import glob
import json
import os
import time

import numpy as np
import pytest

from tests import pystripe_util as U
from tests.conftest import ROOT

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden", U.GOLDEN_SUBDIR)
CASES = sorted(os.path.splitext(os.path.basename(p))[0] for p in glob.glob(os.path.join(GOLD, "*.npz")) if not p.endswith("host.npz"))
PIPE = dict(wavelet="db9", padding_mode="reflect", bidirectional=True)


def report(line):
    print(line)
    path = os.environ.get("PYSTRIPE_REPORT")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def load_case(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    kwargs = json.loads(str(z["kwargs"]))
    for k in ("sigma", "down_sample"):
        if kwargs.get(k) is not None:
            kwargs[k] = tuple(kwargs[k])
    return z, kwargs


@pytest.fixture(scope="module")
def ps(dev):
    from ipp_amd import pystripe
    return pystripe


def check_against(name, got, want, e_ref):
    assert got.shape == want.shape and got.dtype == want.dtype, (got.shape, got.dtype, want.shape, want.dtype)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    if want.dtype.kind in "ui":
        share = float((d != 0).mean())
        report(f"{name}: integer result, {100 * share:.3f} % of pixels differ from the golden, max {d.max():g} counts (E_ref {e_ref:.3g})")
        assert (d <= U.integer_allowance(want, e_ref)).all()
        assert share <= 0.01
    else:
        tol = 5 * e_ref * (np.abs(want.astype(np.float64)) + 1)
        report(f"{name}: float result, max |d| {d.max():.3g}, max d / allowance {(d / np.maximum(tol, 1e-30)).max():.3g}")
        assert (d <= tol).all()


def run_abi(dev, img_stack, params, flat=None):
    """through the C ABI alone: plan_create / plan_info / run / destroy"""
    import torch
    from ipp_amd import capi
    lib = capi.lib()
    n, ny, nx = img_stack.shape
    code = {np.dtype(np.uint8): 0, np.dtype(np.uint16): 1, np.dtype(np.float32): 2}[img_stack.dtype]
    h = C.c_void_p()
    capi.check(lib.mi_pystripe_plan_create(dev.index or 0, ny, nx, code, C.byref(params), C.byref(h)))
    try:
        info = capi.PystripeInfo()
        capi.check(lib.mi_pystripe_plan_info(h, C.byref(info)))
        tin = torch.from_numpy(img_stack).to(dev)
        tdt = {0: torch.uint8, 1: torch.uint16, 2: torch.float32}[info.out_dtype]
        out = torch.full((n, info.out_ny, info.out_nx), 77, dtype=torch.float32, device=dev).to(tdt)
        fl = torch.from_numpy(flat).to(dev) if flat is not None else None
        capi.check(lib.mi_pystripe_run(h, capi.current_stream_ptr(dev), tin.data_ptr(), fl.data_ptr() if fl is not None else None,
                                       out.data_ptr(), n))
        torch.cuda.synchronize(dev)
        return out.cpu().numpy(), info
    finally:
        lib.mi_pystripe_plan_destroy(h)


@pytest.mark.parametrize("name", CASES)
def test_golden_through_process_img(ps, dev, name):
    z, kw = load_case(name)
    flat = z["flat"] if "flat" in z else None
    got = ps.process_img(z["img"].copy(), flat=flat, device=dev, **kw)
    check_against(name, got, z["out"], float(z["e_ref"]) if "e_ref" in z else 0.0)


@pytest.mark.parametrize("name", [c for c in CASES if c not in ("u16_uniform", "u16_nofilter")])
def test_golden_log_domain_through_the_c_abi(ps, dev, name):
    z, kw = load_case(name)
    flat = z["flat"] if "flat" in z else None
    img = z["img"]
    e_ref = float(z["e_ref"])
    prm = ps.make_params(img.dtype, flat=flat is not None, log_output=True, max_batch=2, **kw)
    got, info = run_abi(dev, np.stack([img, img[::-1].copy()]), prm, flat)
    err = float(np.abs(got[0].astype(np.float64) - z["log64"]).max())
    report(f"{name}: log domain, device vs float64 restatement {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f} (allowed 4)")
    assert got.dtype == np.float32 and got[0].shape == z["log64"].shape
    assert err <= 4 * e_ref
    # and the integer / float result of the same plan options through the ABI
    prm = ps.make_params(img.dtype, flat=flat is not None, max_batch=2, **kw)
    out, _ = run_abi(dev, np.stack([img, img[::-1].copy()]), prm, flat)
    check_against(name + " (ABI)", out[0], z["out"], e_ref)


def test_filter_streaks_entry(ps, dev):
    z, kw = load_case("u16_odd_even")
    got = ps.filter_streaks(z["img"].copy(), sigma=kw["sigma"], wavelet="db9", padding_mode="reflect", bidirectional=True, device=dev)
    check_against("filter_streaks", got, z["out"], float(z["e_ref"]))
    log = ps.filter_streaks(z["img"].copy(), sigma=kw["sigma"], wavelet="db9", padding_mode="reflect", bidirectional=True, device=dev,
                            log_output=True)
    assert np.abs(log.astype(np.float64) - z["log64"]).max() <= 4 * float(z["e_ref"])
    # a uniform tile is filtered like any other by filter_streaks (the zero rule belongs to process_img)
    flat_tile = np.full((40, 50), 900, np.uint16)
    got = ps.filter_streaks(flat_tile, sigma=(8, 8), wavelet="db9", padding_mode="reflect", device=dev)
    assert np.abs(got.astype(int) - 900).max() <= 1
    assert not ps.process_img(flat_tile, sigma=(8, 8), wavelet="db9", padding_mode="reflect", device=dev).any()
    # flat field on an integer tile: the stated departure (divided in float32, truncated back to the tile's type)
    rng = np.random.default_rng(5)
    img = U.synthetic_tile((97, 128), 41, np.uint16)
    fl = ps.normalize_flat(0.5 + 0.5 * rng.random(img.shape))
    got = ps.process_img(img, flat=fl, sigma=(16, 16), device=dev, **PIPE)
    want, log64 = U.process_img(img, flat=fl, sigma=(16, 16), dt=np.float64, flat_on_integers=True, **PIPE)
    d = np.abs(got.astype(np.float64) - want.astype(np.float64))
    assert got.dtype == np.uint16 and (d <= U.integer_allowance(want, 5e-6)).all() and (d != 0).mean() <= 0.01


def row_gain_spread(img, axis=1):
    """spread of the per-row (axis=1) or per-column gain estimate: std of log(mean along the line) after removing its smooth part"""
    prof = np.log(img.astype(np.float64).mean(axis=axis) + 1)
    k = 15
    smooth = np.convolve(np.pad(prof, k, mode="edge"), np.ones(2 * k + 1) / (2 * k + 1), mode="valid")
    return float((prof - smooth).std())


def test_structure_row_and_column_stripes(ps, dev):
    z, kw = load_case("u16_big_pipeline")
    e_ref = float(z["e_ref"])
    got = ps.process_img(z["img"].copy(), device=dev, **kw)
    before, gold, after = row_gain_spread(z["img"]), row_gain_spread(z["out"]), row_gain_spread(got)
    report(f"row stripes: gain spread before {before:.4f}, golden {gold:.4f}, device {after:.4f}")
    assert gold < 0.2 * before
    assert after <= gold + 5 * e_ref
    z1, kw1 = load_case("u16_col_stripes_one_dir")
    z2, kw2 = load_case("u16_col_stripes_bidir")
    g1 = ps.process_img(z1["img"].copy(), device=dev, **kw1)
    g2 = ps.process_img(z2["img"].copy(), device=dev, **kw2)
    s0, s1, s2 = row_gain_spread(z1["img"], 0), row_gain_spread(g1, 0), row_gain_spread(g2, 0)
    report(f"column stripes: gain spread before {s0:.4f}, bidirectional=False {s1:.4f}, True {s2:.4f} "
           f"(goldens {row_gain_spread(z1['out'], 0):.4f}, {row_gain_spread(z2['out'], 0):.4f})")
    assert s1 > 0.9 * s0          # left striped (the golden: unchanged to five digits)
    assert s2 < 0.6 * s0          # cleaned (the golden: 0.56 of the spread before, sigma 16 on a 97 x 128 tile)
    assert s2 <= row_gain_spread(z2["out"], 0) + 5 * float(z2["e_ref"])


def test_batch_size_and_position_do_not_matter(ps, dev):
    import torch
    tiles = np.stack([U.synthetic_tile((97, 128), 100 + i, np.uint16, "rows" if i % 2 else "cols") for i in range(16)])
    tiles[5] = 1234      # a uniform tile in the middle of the batch
    outs = {}
    for mb in (1, 3, 16):
        for log in (False, True):
            prm = ps.make_params(np.uint16, sigma=(16, 24), dark=20, rotate=90, log_output=log, max_batch=mb, **PIPE)
            plan = ps.Plan(dev, tiles.shape[1:], np.uint16, prm)
            outs[mb, log] = plan.run(torch.from_numpy(tiles).to(dev)).cpu().numpy()
            plan.close()
    for log in (False, True):
        assert np.array_equal(outs[1, log], outs[3, log]) and np.array_equal(outs[1, log], outs[16, log])
    assert not outs[1, False][5].any() and outs[1, False][4].any()
    # position: the same tile at another place of another batch
    prm = ps.make_params(np.uint16, sigma=(16, 24), dark=20, rotate=90, max_batch=16, **PIPE)
    plan = ps.Plan(dev, tiles.shape[1:], np.uint16, prm)
    perm = np.random.default_rng(0).permutation(16)
    shuffled = plan.run(torch.from_numpy(np.ascontiguousarray(tiles[perm])).to(dev)).cpu().numpy()
    plan.close()
    assert np.array_equal(shuffled, outs[16, False][perm])


@pytest.mark.parametrize("shape,dtype,kw", [
    ((333, 517), np.uint16, dict(sigma=(40, 40), **PIPE)),
    ((260, 131), np.uint8, dict(sigma=(12, 30), wavelet="db9", padding_mode="wrap", bidirectional=True)),
    ((129, 700), np.float32, dict(sigma=(64, 64), wavelet="db9", padding_mode="symmetric", bidirectional=False)),
])
def test_other_shapes_against_the_live_restatement(ps, dev, shape, dtype, kw):
    img = U.synthetic_tile(shape, 7, dtype)
    r32, l32 = U.process_img(img.copy(), dt=np.float32, **kw)
    r64, l64 = U.process_img(img.copy(), dt=np.float64, **kw)
    e_ref = float(np.abs(l32.astype(np.float64) - l64).max())
    log = ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw)
    err = float(np.abs(log.astype(np.float64) - l64).max())
    report(f"live {shape} {np.dtype(dtype).name}: log-domain device {err:.3g}, E_ref (float32 restatement) {e_ref:.3g}, ratio {err / e_ref:.2f}")
    assert err <= 4 * e_ref
    check_against(f"live {shape}", ps.process_img(img.copy(), device=dev, **kw), r32, e_ref)


def test_pipeline_size_2048(ps, dev):
    """2048 x 2048 uint16, sigma (250, 250), reflect, bidirectional: padded 2636 x 2636, 7 levels."""
    img = U.synthetic_tile((2048, 2048), 11, np.uint16)
    kw = dict(sigma=(250, 250), **PIPE)
    t0 = time.perf_counter()
    r32, l32 = U.process_img(img.copy(), dt=np.float32, **kw)
    t1 = time.perf_counter()
    r64, l64 = U.process_img(img.copy(), dt=np.float64, **kw)
    e_ref = float(np.abs(l32.astype(np.float64) - l64).max())
    prm = ps.make_params(np.uint16, log_output=True, **kw)
    assert ps.derive(img.shape, img.dtype, prm).levels == 7
    log = ps.filter_streaks(img.copy(), device=dev, log_output=True, **kw)
    err = float(np.abs(log.astype(np.float64) - l64).max())
    report(f"2048 x 2048 sigma 250: log-domain device {err:.3g}, E_ref {e_ref:.3g}, ratio {err / e_ref:.2f}; "
           f"CPU restatement float32 {t1 - t0:.1f} s per tile (numpy / scipy restatement, not the reference's PyWavelets code)")
    assert err <= 4 * e_ref
    check_against("2048 x 2048 sigma 250", ps.process_img(img.copy(), device=dev, **kw), r32, e_ref)


@pytest.mark.parametrize("max_batch", [64, 4101])
def test_batch_past_2_to_31_samples(ps, dev, max_batch):
    """4101 tiles of 1024 x 1024 uint8 (2^32 + 2^20 samples) in one call.  max_batch 64: the call walks the batch in chunks, the 2^31st
    sample is passed by the host's byte offsets.  max_batch 4101: ONE launch per kernel covers all tiles, so the tile offsets inside
    the kernels pass 2^31 -- in the input and output (tile 2048 on) and inside single scratch buffers (the first level's L / H rows
    hold 1033 x 524 floats per tile: tile 3967 on; the buffers behind the first start beyond 2^31 floats anyway).  Tiles on both sides
    of each boundary, and the last one, equal their single-tile result bit for bit."""
    import torch
    n, ny, nx = 4101, 1024, 1024
    base = np.stack([U.synthetic_tile((ny, nx), 200 + i, np.uint8, "rows") for i in range(3)])
    tin = torch.from_numpy(base).to(dev).repeat(n // 3, 1, 1).contiguous()
    assert tin.numel() > 2 ** 32 and tin.shape[0] == n
    prm = ps.make_params(np.uint8, sigma=(4, 4), wavelet="db9", padding_mode="reflect", bidirectional=True, max_batch=max_batch)
    plan = ps.Plan(dev, (ny, nx), np.uint8, prm)
    info = plan.info
    row_floats = (info.padded_ny + 1) * info.coef_nx[0]
    report(f"2^31 batch, max_batch {max_batch}: scratch {info.scratch_bytes_per_tile / 1e6:.1f} MB per tile, "
           f"{min(max_batch, n) * info.scratch_bytes_per_tile / 1e9:.1f} GB held; first-level row buffer {row_floats} floats per tile")
    if max_batch >= n:
        assert row_floats * (n - 1) > 2 ** 31 and info.scratch_bytes_per_tile // 4 * n > 2 ** 32
    out = plan.run(tin)
    torch.cuda.synchronize(dev)
    plan.close()
    del plan
    one_plan = ps.Plan(dev, (ny, nx), np.uint8, ps.make_params(np.uint8, sigma=(4, 4), wavelet="db9", padding_mode="reflect",
                                                               bidirectional=True, max_batch=3))
    one = one_plan.run(torch.from_numpy(base).to(dev))
    torch.cuda.synchronize(dev)
    one_plan.close()
    edge = 2 ** 31 // row_floats
    for t in (0, 1, 2046, 2047, 2048, 2049, edge - 1, edge, edge + 1, 4099, 4100):
        assert torch.equal(out[t], one[t % 3]), t
    assert out[4100].cpu().numpy().any() and not torch.equal(one[0], one[1])
    del out, tin
    from ipp_amd import capi
    capi.release_cached_memory()


def test_live_plans_with_different_lds_needs(ps, dev):
    """The notch kernel's dynamic-LDS limit belongs to the kernel, not to a plan: plans whose finest lines need 66 176 and 55 872 bytes
    (both above the 48 KB at which the limit has to be raised) and 28 992 bytes of LDS, as Plan.notch_routes() reports them, are alive
    together (as in batch_filter with several tile shapes) and run in turn; every result equals the one the plan gave before the
    others existed.  All three take four lines per work-group; tests/test_gpu_pystripe_notch_routes.py does the same for two and one."""
    import torch
    shapes = [(2048, 2048), (1400, 1400), (300, 300), (1400, 1400), (2048, 2048)]
    kw = dict(sigma=(250, 250), **PIPE)
    tiles = {s: torch.from_numpy(U.synthetic_tile(s, 50, np.uint16)[None]).to(dev) for s in set(shapes)}
    first = {}
    for s in set(shapes):
        plan = ps.Plan(dev, s, np.uint16, ps.make_params(np.uint16, max_batch=1, **kw))
        first[s] = plan.run(tiles[s]).clone()
        torch.cuda.synchronize(dev)
        plan.close()
    plans = {s: ps.Plan(dev, s, np.uint16, ps.make_params(np.uint16, max_batch=1, **kw)) for s in set(shapes)}
    for s in shapes:
        got = plans[s].run(tiles[s])
        torch.cuda.synchronize(dev)
        assert torch.equal(got, first[s]), s
    for plan in plans.values():
        plan.close()


def _write_tiff(path, img):
    from PIL import Image
    path.parent.mkdir(parents=True, exist_ok=True)
    Image.fromarray(img).save(path, format="TIFF", compression="tiff_adobe_deflate")


def test_batch_filter_end_to_end(ps, dev, tmp_path):
    from PIL import Image
    src, dst = tmp_path / "in", tmp_path / "out"
    tiles = {}
    for i in range(5):
        tiles[f"ch0/000100/000100_{i:03d}.tif"] = U.synthetic_tile((97, 128), 300 + i, np.uint16)
    for i in range(3):
        tiles[f"ch0/000200/sub/t_{i:03d}.tiff"] = U.synthetic_tile((75, 101), 310 + i, np.uint16, "cols")
    for rel, img in tiles.items():
        _write_tiff(src / rel, img)
    bad = src / "ch0/000100/000100_bad.tif"
    bad.write_bytes(b"II*\x00 this is not a tiff")
    kw = dict(sigma=(16, 16), dark=30, **PIPE)
    # one output already present: continue_process leaves it alone
    kept = dst / "ch0/000100/000100_000.tif"
    kept.parent.mkdir(parents=True)
    kept.write_bytes(b"already here")
    stats = {}
    assert ps.batch_filter(src, dst, continue_process=True, device=dev, stats=stats, **kw) == 0
    assert kept.read_bytes() == b"already here"
    assert stats["skipped_existing"] == 1 and stats["skipped_unreadable"] == 1 and stats["written"] == 7
    made = sorted(str(p.relative_to(dst)) for p in dst.rglob("*") if p.is_file())
    want_names = sorted(str((dst / rel).with_suffix(".tif").relative_to(dst)) for rel in tiles)
    assert made == want_names
    for rel, img in tiles.items():
        if rel.endswith("000100_000.tif"):
            continue
        with Image.open((dst / rel).with_suffix(".tif")) as im:
            got = np.array(im)
            assert im.info.get("compression") == "tiff_adobe_deflate"
        r32, l32 = U.process_img(img, dt=np.float32, **kw)
        r64, l64 = U.process_img(img, dt=np.float64, **kw)
        e_ref = float(np.abs(l32.astype(np.float64) - l64).max())
        check_against("batch_filter " + rel, got, r32, e_ref)
    # a damaged file with d_type and tile_size: a zero tile; files_list; replacing outputs without continue_process
    dst2 = tmp_path / "out2"
    files = [src / "ch0/000100/000100_bad.tif", src / "ch0/000100/000100_001.tif"]
    assert ps.batch_filter(src, dst2, files_list=files, d_type="uint16", tile_size=(97, 128), rotate=90, device=dev, **kw) == 0
    with Image.open(dst2 / "ch0/000100/000100_bad.tif") as im:
        z = np.array(im)
    assert z.shape == (128, 97) and z.dtype == np.uint16 and not z.any()
    # a 2-rank torchrun-style split covers every file once
    dst3 = tmp_path / "out3"
    env = dict(os.environ)
    try:
        counts = []
        for rank in range(2):
            os.environ.update(RANK=str(rank), WORLD_SIZE="2", LOCAL_RANK="0")
            st = {}
            assert ps.batch_filter(src, dst3, device=dev, stats=st, **kw) == 0
            counts.append(st["written"])
    finally:
        os.environ.clear()
        os.environ.update(env)
    assert sum(counts) == 8 and min(counts) >= 3
    assert sorted(str(p.relative_to(dst3)) for p in dst3.rglob("*.tif")) == want_names
