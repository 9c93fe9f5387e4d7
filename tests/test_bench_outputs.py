"""CPU: what ``bench.py --dump-outputs`` writes (bench.output_sample / bench.dump_outputs) on small host volumes: the arrays of
the whole volume, the same arrays summed over y slabs (N > 1: every rank contributes its rows), the size bound of every workload."""
import os

import numpy as np
import pytest
import torch

import bench


def _vol(shape, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).random(shape, dtype=np.float32))


def test_small_volume_is_written_whole():
    vol = _vol((6, 10, 12))
    out = bench.output_sample(vol, tuple(vol.shape))
    assert out["deconvolved_sample"].dtype == torch.float32 and torch.equal(out["deconvolved_sample"], vol.reshape(-1))
    assert torch.equal(out["deconvolved_mid_plane"], vol[3])
    assert out["deconvolved_plane_sums"].dtype == torch.float64
    assert torch.allclose(out["deconvolved_plane_sums"], vol.double().sum(dim=(1, 2)), rtol=1e-12, atol=0)


def test_large_volume_is_sampled_at_seeded_indices(monkeypatch):
    monkeypatch.setattr(bench, "DUMP_WHOLE", 100)
    monkeypatch.setattr(bench, "DUMP_SAMPLES", 300)
    monkeypatch.setattr(bench, "DUMP_PLANE", 6)
    vol = _vol((7, 9, 11), seed=1)
    n = vol.numel()
    idx = np.unique(np.random.default_rng(bench.DUMP_SEED).integers(0, n, 300))
    out = bench.output_sample(vol, tuple(vol.shape))
    assert torch.equal(out["deconvolved_sample"], vol.reshape(-1)[torch.from_numpy(idx)])
    assert torch.equal(out["deconvolved_mid_plane"], vol[3, 1:7, 2:8])       # cropped about the centre: (9 - 6) // 2, (11 - 6) // 2
    again = bench.output_sample(vol.clone(), tuple(vol.shape))
    assert all(torch.equal(out[k], again[k]) for k in out)


@pytest.mark.parametrize("whole", [True, False], ids=["whole", "sampled"])
def test_slabs_sum_to_the_whole_volume(monkeypatch, whole):
    if not whole:
        monkeypatch.setattr(bench, "DUMP_WHOLE", 100)
        monkeypatch.setattr(bench, "DUMP_SAMPLES", 500)
        monkeypatch.setattr(bench, "DUMP_PLANE", 8)
    vol = _vol((5, 13, 10), seed=2)
    want = bench.output_sample(vol, tuple(vol.shape))
    parts = [bench.output_sample(vol[:, a:b], tuple(vol.shape), a) for a, b in ((0, 4), (4, 5), (5, 13))]
    for k in ("deconvolved_sample", "deconvolved_mid_plane"):
        assert torch.equal(sum(p[k] for p in parts), want[k]), k
    assert torch.allclose(sum(p["deconvolved_plane_sums"] for p in parts), want["deconvolved_plane_sums"], rtol=1e-12, atol=0)


def test_dump_files_and_size_bound(tmp_path):
    vol = _vol((4, 6, 8), seed=3)
    bench.dump_outputs(str(tmp_path / "out"), bench.output_sample(vol, tuple(vol.shape)))
    got = {f: np.load(tmp_path / "out" / f) for f in sorted(os.listdir(tmp_path / "out"))}
    assert sorted(got) == ["deconvolved_mid_plane.npy", "deconvolved_plane_sums.npy", "deconvolved_sample.npy"]
    assert got["deconvolved_sample.npy"].dtype == np.float32 and got["deconvolved_plane_sums.npy"].dtype == np.float64
    assert np.array_equal(got["deconvolved_sample.npy"], vol.numpy().reshape(-1))
    for name, (shape, _) in bench.WORKLOADS.items():    # at most 64 MB for every workload of the bench
        n = int(np.prod(shape))
        nbytes = 4 * min(n, bench.DUMP_SAMPLES if n > bench.DUMP_WHOLE else n) + 4 * min(shape[1], bench.DUMP_PLANE) * \
            min(shape[2], bench.DUMP_PLANE) + 8 * shape[0]
        assert nbytes <= 64 << 20, (name, nbytes)
