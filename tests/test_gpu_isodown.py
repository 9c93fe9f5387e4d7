"""GPU: the isotropic down-sampling (include/mi_isodown.h, ipp_amd.parallel_image_processor) against the restatement of
tests/isodown_util.py.

The standard: the halving chain and the z reduction are EQUAL to the restatement bit by bit (max and the two-term float32 mean are
exact operations); planes, ``mi_resize_antialias`` and ``I`` are within 2e-6 x max|input| of it (ten times the distance of a
float32-accumulating separable form from scipy's own filter + zoom, measured on the CPU: tests/test_isodown_host.py); ``xI`` and
the full-resolution files are equal.  Every figure is printed before it is asserted.
"""
import os

import numpy as np
import pytest

from tests import isodown_util as U

pytestmark = pytest.mark.gpu
TOL = 2e-6
SIX = ["A", "B", "C", "D", "E", "F"]
DTYPES = [np.uint8, np.uint16, np.float32]


def report(line):
    print("[isodown] " + line, flush=True)


@pytest.fixture(scope="module")
def pip():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import parallel_image_processor
    return parallel_image_processor


@pytest.fixture(scope="module")
def ps(pip):
    from ipp_amd import pystripe
    return pystripe


def make_plan(pip, dev, name, dtype, alternating=True, **kw):
    shape, voxel, target = U.CASES[name]
    return pip.Plan(dev, shape, dtype, voxel, target, alternating, **kw)


def within(got, want, top, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max()) / float(top)
    report(f"{what}: max abs error {err:.3e} of max|input| (bound {TOL:.0e})")
    assert got.shape == want.shape
    assert err <= TOL, (what, err)
    return err


# ---------------------------------------------------------------------------------------------------------------------------------
# the halving chain alone

@pytest.mark.parametrize("alternating", [True, False], ids=["alternating", "mean"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_halving_chain_is_bit_identical(pip, dev, name, dtype, alternating):
    import torch
    shape, voxel, target = U.CASES[name]
    stack = np.stack([U.pattern(shape, dtype, seed) for seed in (1, 2)])
    want_plan = U.plan(shape, voxel, target, alternating)
    plan = make_plan(pip, dev, name, dtype, alternating)
    try:
        assert plan.info["steps"] == want_plan["steps"] and plan.halved_shape == want_plan["halved_shape"]
        halved, differs = plan.halve(torch.from_numpy(stack).to(dev))
        halved, differs = halved.cpu().numpy(), differs.cpu().numpy()
    finally:
        plan.close()
    for k in range(2):
        want = U.halve_chain(stack[k], want_plan)
        assert halved[k].dtype == np.float32 and np.array_equal(halved[k], want), (name, k, np.abs(halved[k] - want).max())
    assert differs.tolist() == [1, 1]


def test_uniform_flag_and_zero_plane(pip, dev):
    import torch
    for name in ("A", "V"):
        shape, voxel, target = U.CASES[name]
        uniform = np.full(shape, 700, np.uint16)
        last = uniform.copy()
        last[-1, -1] = 701   # one differing sample, the last one
        first_row = uniform.copy()
        first_row[0, 1] = 3
        stack = np.stack([uniform, last, U.pattern(shape, np.uint16, 4), first_row])
        p = U.plan(shape, voxel, target)
        plan = make_plan(pip, dev, name, np.uint16)
        try:
            _, differs = plan.halve(torch.from_numpy(stack).to(dev))
            planes = plan.planes(torch.from_numpy(stack).to(dev)).cpu().numpy()
        finally:
            plan.close()
        assert differs.cpu().numpy().tolist() == [0, 1, 1, 1]
        assert not planes[0].any()
        for k in range(4):
            within(planes[k], U.slice_plane(stack[k], p), max(1.0, float(stack[k].max())), f"case {name} plane {k} beside a uniform slice")
        assert planes[1].any()


# ---------------------------------------------------------------------------------------------------------------------------------
# whole slice plane, mi_resize_antialias

@pytest.mark.parametrize("dtype", [np.uint16, np.float32], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("name", sorted(U.CASES))
def test_slice_plane(pip, dev, name, dtype):
    import torch
    shape, voxel, target = U.CASES[name]
    stack = np.stack([U.pattern(shape, dtype, seed) for seed in (5, 6, 7)])
    p = U.plan(shape, voxel, target)
    plan = make_plan(pip, dev, name, dtype, max_group=2)   # three slices through scratch for two
    try:
        assert plan.target_shape == p["target_shape"]
        planes = plan.planes(torch.from_numpy(stack).to(dev)).cpu().numpy()
    finally:
        plan.close()
    for k in range(3):
        halved = U.halve_chain(stack[k], p)
        within(planes[k], U.slice_plane(stack[k], p), np.abs(halved).max(), f"case {name} {np.dtype(dtype).name} slice {k} plane {p['target_shape']}")


@pytest.mark.parametrize("name", SIX)
def test_resize_antialias_2d(pip, dev, name):
    p = U.plan(*U.CASES[name])
    a = np.random.default_rng(8).uniform(-300, 4000, p["halved_shape"]).astype(np.float32)
    got = pip.resize_antialias(a, p["target_shape"], dev)
    within(got, U.resize(a, p["target_shape"]), np.abs(a).max(), f"mi_resize_antialias {p['halved_shape']} -> {p['target_shape']}")


@pytest.mark.parametrize("shapes", [((7, 33, 29), (3, 20, 29)), ((5, 12, 12), (5, 12, 12))], ids=["shrink", "same"])
def test_resize_antialias_3d(pip, dev, shapes):
    src, dst = shapes
    a = np.random.default_rng(9).uniform(-300, 4000, src).astype(np.float32)
    got = pip.resize_antialias(a, dst, dev)
    within(got, U.resize(a, dst), np.abs(a).max(), f"mi_resize_antialias {src} -> {dst}")
    if src == dst:
        assert np.array_equal(got, a)


def test_resize_refusals(pip, dev):
    from ipp_amd import capi
    a = np.ones((5000, 2), np.float32)
    with pytest.raises(capi.MiError) as e:
        pip.resize_antialias(a, (2, 2), dev)   # sigma 1249.5: a radius of 4998
    assert e.value.code == capi.MI_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        pip.resize_antialias(a, (0, 2), dev)


# ---------------------------------------------------------------------------------------------------------------------------------
# z reduction, conversions

@pytest.mark.parametrize("n,rounds", [(1, 1), (2, 2), (3, 2), (5, 3), (10, 4)])
def test_z_reduction_is_bit_identical(pip, dev, n, rounds):
    import torch
    rng = np.random.default_rng(n)
    stack = rng.uniform(-50, 900, (n, 19, 23)).astype(np.float32)
    plane, uniform = pip.reduce_z(torch.from_numpy(stack).to(dev), rounds)
    assert int(uniform.item()) == 0
    assert np.array_equal(plane.cpu().numpy(), U.z_reduce(stack, rounds))
    same = np.full((n, 19, 23), 12.5, np.float32)
    plane, uniform = pip.reduce_z(torch.from_numpy(same).to(dev), rounds)
    assert int(uniform.item()) == 1 and not plane.cpu().numpy().any()
    if n == 10:
        with pytest.raises(ValueError):
            pip.reduce_z(torch.from_numpy(stack).to(dev), 3)   # 10 -> 5 -> 3 -> 2


def test_group_run_and_conversions(pip, dev):
    """one z group of case A through mi_isodown_run: a full group of two and the short last group of one, float32 / uint16 / uint8"""
    import torch
    shape, voxel, target = U.CASES["A"]
    p = U.plan(shape, voxel, target)
    for dtype in (np.uint16, np.uint8):
        for n in (2, 1):
            stack = np.stack([U.pattern(shape, dtype, 20 + k) for k in range(n)])
            want_stack = np.stack([U.slice_plane(s, p) for s in stack])
            got = {}
            for out in ("float32", "uint16", "uint8"):
                plan = make_plan(pip, dev, "A", dtype, z_rounds=2, out_dtype=out, max_group=2)
                try:
                    plane, uniform = plan.run(torch.from_numpy(stack).to(dev))
                    got[out] = plane.cpu().numpy()
                    assert int(uniform.item()) == 0
                finally:
                    plan.close()
            within(got["float32"], U.z_reduce(want_stack, 2), float(stack.max()), f"group of {n} {np.dtype(dtype).name} slices")
            # the conversions are exact functions of the float32 plane
            for out in ("uint16", "uint8"):
                want = U.z_reduce(np.stack([got["float32"], got["float32"]]), 1, out, dtype)
                assert got[out].dtype == np.dtype(out) and np.array_equal(got[out], want), (dtype, n, out)
            assert got["uint16"].max() > 255 or dtype == np.uint8


# ---------------------------------------------------------------------------------------------------------------------------------
# end to end

VOXEL, TARGET, COUNT = (2.0, 1.0, 0.5), 5.0, 23


@pytest.fixture(scope="module")
def folder(ps, tmp_path_factory):
    root = tmp_path_factory.mktemp("isodown")
    src = root / "stitched"
    src.mkdir()
    slices = [U.pattern((45, 70), np.uint16, 100 + i) for i in range(COUNT)]
    slices[7] = np.full((45, 70), 300, np.uint16)   # a uniform slice inside a group
    for i, s in enumerate(slices):
        ps.imsave_tif(src / f"s_{i}.tif", s)        # natural order: s_2 before s_10
    return root, src, slices


def read_planes(ps, folder_path):
    return [ps.imread_tif_raw_png(f) for f in sorted(folder_path.glob("*.tif"))]


def check_products(ps, pip, dest, ds_dir, want, tag, where=None):
    where = dest if where is None else where   # downsampled_path defaults to the destination, as in the reference
    assert ds_dir == where / f"{dest.name}_z4.0_yx5.0um"
    planes = read_planes(ps, ds_dir)
    assert [f.name for f in sorted(ds_dir.glob("*"))] == [f"img_{g:06}.tif" for g in range(12)]
    top = max(float(np.abs(s).max()) for s in want["processed"])
    for g, (got, ref) in enumerate(zip(planes, want["planes"])):
        assert got.dtype == ref.dtype
        err = float(np.abs(got.astype(np.float64) - ref).max()) / top
        assert err <= TOL, (tag, g, err)
    npz = np.load(where / f"{dest.name}_zyx5.0um.npz", allow_pickle=True)
    assert npz["I"].dtype == want["I"].dtype
    within(npz["I"], want["I"], top, f"{tag}: I {npz['I'].shape}")
    assert len(npz["xI"]) == 3
    for got, ref in zip(npz["xI"], want["xI"]):
        assert got.dtype == np.float64 and np.array_equal(got, ref)


def test_folder_without_fun(ps, pip, folder):
    root, src, slices = folder
    dest = root / "plain"
    rc, ds_dir = pip.parallel_image_processor(src, dest, source_voxel=VOXEL, target_voxel=TARGET, return_downsampled_path=True)
    assert rc == 0 and list(dest.glob("*.tif")) == []   # nothing to write at full resolution
    check_products(ps, pip, dest, ds_dir, U.run_folder(slices, VOXEL, TARGET), "fun=None")
    assert pip.parallel_image_processor(src, dest, source_voxel=VOXEL, target_voxel=TARGET) == 0


def test_folder_through_process_img(ps, pip, folder):
    root, src, slices = folder
    dest = root / "processed"
    kw = dict(dark=120, convert_to_8bit=True, bit_shift_to_right=8)
    rc, ds_dir = pip.parallel_image_processor(src, dest, fun=ps.process_img, kwargs=kw, source_voxel=VOXEL, target_voxel=TARGET,
                                              return_downsampled_path=True)
    assert rc == 0
    want = U.run_folder(slices, VOXEL, TARGET, fun=lambda img: ps.process_img(img, **kw))
    assert want["processed"][0].dtype == np.uint8
    check_products(ps, pip, dest, ds_dir, want, "fun=process_img")
    for i, ref in enumerate(want["processed"]):
        got = ps.imread_tif_raw_png(dest / f"s_{i}.tif")
        assert got.dtype == ref.dtype and np.array_equal(got, ref), i


def test_folder_rotated(ps, pip, folder):
    root, src, slices = folder
    dest = root / "rotated"
    rc, ds_dir = pip.parallel_image_processor(src, dest, source_voxel=VOXEL, target_voxel=TARGET, rotation=90, rename=True,
                                              downsampled_path=root, return_downsampled_path=True)
    assert rc == 0
    want = U.run_folder(slices, VOXEL, TARGET, rotation=90)
    assert want["target_shape_3d"] == [9, 7, 9] and want["planes"][0].shape == (7, 9)
    check_products(ps, pip, dest, ds_dir, want, "rotation=90", where=root)
    for i, s in enumerate(slices):
        assert np.array_equal(ps.imread_tif_raw_png(dest / f"img_{i:06}.tif"), np.rot90(s))


def test_folder_converted_planes(ps, pip, folder):
    """down_sampled_dtype uint16 / uint8 through the Python entry: the planes are the conversions of the float32 run's planes (values
    2e-6 apart may truncate to neighbouring integers), I is float64"""
    root, src, slices = folder
    for name in ("uint16", "uint8"):
        dest = root / f"as_{name}"
        _, ds_dir = pip.parallel_image_processor(src, dest, source_voxel=VOXEL, target_voxel=TARGET, down_sampled_dtype=name,
                                                 return_downsampled_path=True)
        want = U.run_folder(slices, VOXEL, TARGET, out_dtype=name)
        for g, (got, ref) in enumerate(zip(read_planes(ps, ds_dir), want["planes"])):
            assert got.dtype == ref.dtype == np.dtype(name) and got.shape == ref.shape
            assert np.abs(got.astype(np.int64) - ref.astype(np.int64)).max() <= 1, (name, g)
        volume = np.load(dest / f"as_{name}_zyx5.0um.npz", allow_pickle=True)["I"]
        assert volume.dtype == np.float64 and volume.shape == (9, 9, 7)
        assert np.abs(volume - want["I"]).max() <= 1.0 + TOL * 65535


def test_resume_rewrites_only_what_is_missing(ps, pip, folder):
    root, src, slices = folder
    dest = root / "resumed"
    kw = dict(dark=120, convert_to_8bit=True, bit_shift_to_right=8)
    call = dict(fun=ps.process_img, kwargs=kw, source_voxel=VOXEL, target_voxel=TARGET, return_downsampled_path=True)
    _, ds_dir = pip.parallel_image_processor(src, dest, **call)
    npz_file = dest / "resumed_zyx5.0um.npz"
    before = {f: (f.stat().st_mtime_ns, f.read_bytes()) for f in list(ds_dir.glob("*.tif")) + list(dest.glob("*.tif"))}
    volume = np.load(npz_file, allow_pickle=True)["I"]
    gone = ds_dir / "img_000003.tif"
    gone.unlink()
    npz_file.unlink()
    os.utime(dest / "s_6.tif", ns=(1, 1))   # a full-resolution file of that group: it must be read back, not written again
    pip.parallel_image_processor(src, dest, **call)
    assert gone.exists() and npz_file.exists()
    assert (dest / "s_6.tif").stat().st_mtime_ns == 1
    for f, (mtime, content) in before.items():
        assert f.read_bytes() == content, f
        if f != gone and f.name != "s_6.tif":
            assert f.stat().st_mtime_ns == mtime, f"{f} was written again"
    assert np.array_equal(np.load(npz_file, allow_pickle=True)["I"], volume)
    # an existing npz ends the call: planes that are missing then stay missing only if their group is complete -- here nothing is
    stamp = npz_file.stat().st_mtime_ns
    pip.parallel_image_processor(src, dest, **call)
    assert npz_file.stat().st_mtime_ns == stamp


def test_refused_geometry_before_any_work(pip, folder):
    root, src, _ = folder
    dest = root / "refused"
    with pytest.raises(ValueError, match="rounds along z"):
        pip.parallel_image_processor(src, dest, source_voxel=(1.0, 1.0, 0.5), target_voxel=9.0)
    assert not list(dest.glob("*"))
    with pytest.raises(ValueError):
        pip.parallel_image_processor(src, dest, source_voxel=(2.0, 1.0, 0.5), target_voxel=80.0)
    assert not list(dest.parent.glob("refused_*"))
