"""CPU: the host side of the isotropic down-sampling (include/mi_isodown.h, ipp_amd.parallel_image_processor) against the restatement
of tests/isodown_util.py: the plan of a slice shape, z groups and rounds, the departures from the reference, refusals, ``xI``, names,
and the restatement's ``resize`` against its own separable form (the form the kernels compute)."""
import math
import os

import numpy as np
import pytest

from tests import isodown_util as U


@pytest.fixture(scope="module")
def pip():
    import __graft_entry__ as g
    g.build()
    from ipp_amd import parallel_image_processor
    return parallel_image_processor


def same_plan(pip, shape, voxel, target, alternating):
    want = U.plan(shape, voxel, target, alternating)
    got = pip.derive(shape, voxel, target, alternating)
    assert got["target_shape"] == want["target_shape"], (shape, voxel, target, got, want)
    assert got["steps"] == want["steps"], (shape, voxel, target, got["steps"], want["steps"])
    assert got["halved_shape"] == want["halved_shape"]
    if alternating:
        assert got["rounds"] == want["factors"]
    for axis in (0, 1):
        f = want["halved_shape"][axis] / want["target_shape"][axis]
        sigma = max(0.0, (f - 1) / 2)
        assert got["sigma"][axis] == sigma
        radius = int(4 * sigma + 0.5) if sigma > 1e-15 else 0
        assert got["radius"][axis] == radius
        assert got["taps"][axis] == (2 * radius + 1 if sigma > 1e-15 else 0)
    # the kernel's tile: powers of two whose source block fits its LDS
    ty, tx = got["tile"]
    ky, kx = (sum(1 for s in want["steps"] if s[0] == axis) for axis in (0, 1))
    if (ty, tx) == (0, 0):   # only a target extent of 1 keeps halving that far: the block behind one sample is past the kernel's LDS
        assert 2 ** (ky + kx) > 8192 and 1 in want["target_shape"]
    else:
        assert ty >= 1 and tx >= 1 and ty & (ty - 1) == 0 and tx & (tx - 1) == 0
    assert got["scratch_bytes_per_slice"] >= 4 * (3 * np.prod(want["halved_shape"]) + np.prod(want["target_shape"]))
    return got


@pytest.mark.parametrize("name", sorted(U.CASES))
@pytest.mark.parametrize("alternating", [True, False])
def test_derive_equals_the_restatement_on_the_cases(pip, name, alternating):
    shape, voxel, target = U.CASES[name]
    same_plan(pip, shape, voxel, target, alternating)


def test_the_cases_reach_what_they_are_meant_to(pip):
    a = pip.derive(*U.CASES["A"])
    assert a["rounds"] == (2, 3) and a["halved_shape"] == (12, 9) and a["target_shape"] == (9, 7)
    assert (0, "mean", 23) in a["steps"] and (1, "max", 35) in a["steps"]
    b = pip.derive(*U.CASES["B"])
    assert b["rounds"] == (3, 3) and b["halved_shape"] == (5, 6) and b["target_shape"] == (3, 3)
    assert all(extent % 2 for _, _, extent in b["steps"][:4])
    c = pip.derive(*U.CASES["C"])
    assert c["steps"] == [] and c["target_shape"] == (7, 22) and c["sigma"][1] == 0.25 and c["radius"] == (1, 1)
    d = pip.derive(*U.CASES["D"])
    assert d["rounds"] == (5, 5) and d["halved_shape"] == (3, 4) and d["target_shape"] == (3, 3)
    e = pip.derive(*U.CASES["E"])
    assert e["steps"] == [] and e["target_shape"] == (18, 14) and e["taps"] == (0, 0)
    f = pip.derive(*U.CASES["F"])
    assert f["rounds"] == (2, 1) or f["rounds"][0] > f["rounds"][1]
    assert f["radius"][1] >= f["halved_shape"][1] or f["halved_shape"][1] <= 3


def test_derive_equals_the_restatement_on_a_sweep(pip):
    rng = np.random.default_rng(11)
    done = 0
    while done < 200:
        shape = (int(rng.integers(1, 401)), int(rng.integers(1, 401)))
        voxel = (float(rng.choice([0.4, 0.5, 0.7, 1.0, 1.3, 2.0, 3.7])), float(rng.choice([0.4, 0.5, 0.7, 1.0, 1.3, 2.0, 3.7])))
        target = float(rng.choice([1.0, 1.5, 2.9, 5.0, 10.0, 25.0, 30.0, 50.0]))
        want = U.plan(shape, voxel, target)
        if min(want["target_shape"]) < 1:
            with pytest.raises(ValueError):
                pip.derive(shape, voxel, target)
            continue
        same_plan(pip, shape, voxel, target, bool(done % 2))
        done += 1


def test_scaled_voxel_of_a_changed_and_a_rotated_shape(pip):
    for source, new, rotated in (((45, 70), (45, 70), False), ((45, 70), (23, 35), False), ((45, 70), (70, 45), True), ((45, 70), (35, 23), True)):
        assert pip.scaled_voxel(source, (2.0, 1.0, 0.5), new, rotated) == U.scaled_voxel(source, (2.0, 1.0, 0.5), new, rotated)


def test_z_groups_and_rounds(pip):
    for target, vz in ((5.0, 2.0), (10.0, 0.7), (10.0, 10.0), (10.0, 25.0), (10.0, 3.0), (7.0, 1.0)):
        assert pip.z_steps(target, vz) == U.z_steps(target, vz) == max(1, math.floor(target / vz))
        assert pip.z_rounds(target, vz) == U.z_rounds(target, vz)
    assert pip.z_groups(23, 2) == U.z_groups(23, 2)
    assert pip.z_groups(23, 2)[-1] == [22] and len(pip.z_groups(23, 2)) == 12
    assert pip.z_groups(5, 1) == [[0], [1], [2], [3], [4]]
    rng = np.random.default_rng(3)
    for n, rounds in ((1, 1), (2, 2), (3, 2), (5, 3), (10, 4)):
        stack = rng.uniform(-5, 50, (n, 4, 5)).astype(np.float32)
        got = U.z_reduce(stack, rounds)
        assert got.shape == (4, 5) and got.dtype == np.float32
    assert not U.z_reduce(np.full((3, 4, 5), 7, np.float32), 2).any()   # a uniform stack gives zeros
    pair = np.stack([np.full((2, 2), 3, np.float32), np.array([[1, 5], [2, 9]], np.float32)])
    assert np.array_equal(U.z_reduce(pair, 1), np.maximum(pair[0], pair[1]))
    three = np.stack([pair[0], pair[1], pair[1] * 4])
    # round 0: max of the first two, max(third, 0); round 1: their mean
    assert np.array_equal(U.z_reduce(three, 2), (np.maximum(pair[0], pair[1]) + pair[1] * 4) / 2)


def test_departure_last_group_holds_only_slices_that_exist(pip):
    # count mod steps == steps - 1: the reference's last group names index `count`
    ref = U.z_groups_of_the_reference(0, 11, 4)
    assert ref[-1] == [8, 9, 10, 11]
    assert pip.z_groups(11, 4)[-1] == [8, 9, 10]
    for count in range(1, 30):
        for steps in range(1, 8):
            groups = pip.z_groups(count, steps)
            assert [i for g in groups for i in g] == list(range(count))
            if count % steps != steps - 1 or steps == 1:
                assert groups == U.z_groups_of_the_reference(0, count, steps)


def test_departure_geometry_the_reference_stops_on(pip, tmp_path):
    bad = [s for s in range(1, 201) if pip.planes_left(s, pip.z_rounds(float(s), 1.0)) != 1]
    assert bad == [9]
    pip.check_z_geometry(23, 5.0, 2.0)
    pip.check_z_geometry(40, 10.0, 0.7)
    with pytest.raises(ValueError, match="rounds along z"):
        pip.check_z_geometry(40, 9.0, 1.0)
    pip.check_z_geometry(8, 9.0, 1.0)   # eight planes reduce to one in three rounds
    with pytest.raises(ValueError, match="rounds"):
        U.z_reduce(np.arange(9 * 4, dtype=np.float32).reshape(9, 2, 2), 3)


def test_departure_target_extent_of_zero(pip):
    with pytest.raises(ValueError, match="rounds to"):
        pip.derive((3, 40), (1.0, 1.0), 10.0)
    with pytest.raises(ValueError):
        pip.volume_target_shape(2, (40, 40), (1.0, 1.0, 1.0), 10.0)
    assert pip.volume_target_shape(23, (45, 70), (2.0, 1.0, 0.5), 5.0) == U.volume_target_shape(23, (45, 70), (2.0, 1.0, 0.5), 5.0) == [9, 9, 7]
    assert pip.volume_target_shape(23, (45, 70), (2.0, 1.0, 0.5), 5.0, 90) == [9, 7, 9]


def test_refused_sources(pip, tmp_path):
    class TSVVolume:
        pass
    with pytest.raises(NotImplementedError, match="TSVVolume"):
        pip.parallel_image_processor(TSVVolume(), tmp_path / "out")
    with pytest.raises(NotImplementedError, match="ims"):
        pip.parallel_image_processor(tmp_path / "volume.ims", tmp_path / "out")
    with pytest.raises(NotImplementedError, match="ims"):
        pip.parallel_image_processor(str(tmp_path / "VOLUME.IMS"), tmp_path / "out")


def test_xi_equals_the_restatement(pip):
    for count, shape, voxel, target, rotation in ((23, (45, 70), (2.0, 1.0, 0.5), 5.0, 0), (23, (45, 70), (2.0, 1.0, 0.5), 5.0, 90),
                                                  (40, (37, 41), (0.7, 0.7, 0.7), 10.0, 0), (7, (9, 7), (2.0, 2.0, 2.0), 1.0, 0)):
        t3 = pip.volume_target_shape(count, shape, voxel, target, rotation)
        got = pip.generate_voxel_spacing((count,) + shape, voxel, t3, target)
        want = U.generate_voxel_spacing((count,) + shape, voxel, t3, target)
        assert len(got) == 3
        for g, w, m in zip(got, want, t3):
            assert g.dtype == np.float64 and g.shape == (m,) and np.array_equal(g, w)
    # element 0 of the local mean: the first n / m inputs, the last one by the part of it inside
    assert U.local_mean_first([1.0, 2.0, 3.0, 4.0], 2) == 1.5
    assert U.local_mean_first([1.0, 2.0, 4.0], 2) == pytest.approx((1.0 + 0.5 * 2.0) / 1.5)
    assert U.local_mean_first([1.0, 2.0], 4) == 1.0
    assert pip.local_mean_first([1.0, 2.0, 4.0], 2) == U.local_mean_first([1.0, 2.0, 4.0], 2)


def test_directory_and_file_names(pip, tmp_path):
    dest = tmp_path / "stitched_Ex_561"
    assert pip.downsampled_dir(tmp_path, dest, 2, 2.0, 5.0).name == "stitched_Ex_561_z4.0_yx5.0um"
    assert pip.downsampled_dir(tmp_path, dest, 14, 0.7, 10).name == f"stitched_Ex_561_z{14 * 0.7:.1f}_yx10.0um"
    assert pip.npz_path(tmp_path, dest, 10.0) == tmp_path / "stitched_Ex_561_zyx10.0um.npz"
    images = ["/data/in/a_2.tif", "/data/in/a_10.raw", "/data/in/b.PNG", "/data/in/c.tiff"]
    assert pip.tif_save_path(dest, images, 0) == dest / "a_2.tif"
    assert pip.tif_save_path(dest, images, 1) == dest / "a_10.tif"
    assert pip.tif_save_path(dest, images, 2) == dest / "b.tif"
    assert pip.tif_save_path(dest, images, 3) == dest / "c.tiff"
    assert pip.tif_save_path(dest, images, 3, rename=True, tif_prefix="img") == dest / "img_000003.tif"
    assert pip.natural_sorted(["s_10.tif", "s_9.tif", "s_100.tif", "s_1.tif"]) == ["s_1.tif", "s_9.tif", "s_10.tif", "s_100.tif"]


def test_command_line_options(pip):
    a = pip._parse_args(["--input", "in", "--output", "out", "--voxel_size", "2", "1", "0.5", "--voxel_size_target", "5", "--no-alternating",
                         "--rotation", "90", "--down_sampled_dtype", "uint16", "--rename"])
    assert a.voxel_size == [2.0, 1.0, 0.5] and a.voxel_size_target == 5.0 and a.alternating is False and a.rotation == 90 and a.rename
    assert a.down_sampled_dtype == "uint16" and a.downsampled_path is None


RESIZES = [((45, 70), (9, 7)), ((12, 9), (9, 7)), ((10, 33), (7, 22)), ((9, 7), (18, 14)), ((19, 1), (5, 1)), ((19, 3), (5, 3)),
           ((7, 33, 29), (3, 20, 29)), ((5, 12, 12), (5, 12, 12)), ((4, 9, 30), (6, 5, 11))]


@pytest.mark.parametrize("shapes", RESIZES, ids=lambda s: "x".join(map(str, s[0])) + "-" + "x".join(map(str, s[1])))
def test_resize_is_separable(shapes):
    """per-axis taps on all axes, then per-axis two-point interpolation on all axes, reproduce scipy's filter + zoom (up-sampling on
    one axis and an extent of 1 included).  Every pass is a convex combination, so an error never grows from pass to pass and every
    float32 rounding adds at most 2^-24 of the largest sample: with float64 accumulation one rounding per stored axis result
    (2 ndim stores), with float32 accumulation about sixteen (the bound of the GPU test, 2e-6, is ten times what was seen here)."""
    src, dst = shapes
    a = np.random.default_rng(5).uniform(-200, 3000, src).astype(np.float32)
    want = U.resize(a, dst)
    top = np.abs(a).max()
    e64 = np.abs(U.resize_separable(a, dst, np.float64) - want).max() / top
    e32 = np.abs(U.resize_separable(a, dst, np.float32) - want).max() / top
    print(f"[isodown] separable resize {src} -> {dst}: float64 accumulation {e64:.2e}, float32 accumulation {e32:.2e} of max|a|")
    assert e64 <= 2 * len(src) * 2.0 ** -24 and e32 <= 16 * 2.0 ** -24
    assert want.min() >= a.min() and want.max() <= a.max()


def test_halve_pads_zeros_behind_an_odd_extent():
    a = np.array([[1, 2, 3], [4, 5, 6], [7, 8, 10]], np.float32)
    assert np.array_equal(U.halve(a, 0, "max"), [[4, 5, 6], [7, 8, 10]])
    assert np.array_equal(U.halve(a, 0, "mean"), [[2.5, 3.5, 4.5], [3.5, 4, 5]])
    assert np.array_equal(U.halve(a, 1, "mean"), [[1.5, 1.5], [4.5, 3], [7.5, 5]])
    assert np.array_equal(U.halve(-a, 1, "max"), [[-1, 0], [-4, 0], [-7, 0]])   # the pad is zero, whatever the data
