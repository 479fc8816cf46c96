"""bench.py --dump-outputs without a GPU: the writer keeps small outputs whole, samples large ones to the same seeded
elements every time, and stays under the 64 MB budget."""
import os

import numpy as np
import torch

import bench


def test_small_outputs_are_written_whole(tmp_path):
    a, b = torch.randn(2, 2, 8, 12), torch.randn(2, 2, 8, 12)
    rec = bench.dump_outputs({"img": a, "x_start": b}, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["img.npy", "x_start.npy"]
    for n, t in (("img", a), ("x_start", b)):
        x = np.load(tmp_path / f"{n}.npy")
        assert x.dtype == np.float32 and np.array_equal(x, t.numpy())
        assert rec["files"][f"{n}.npy"] == {"shape": [2, 2, 8, 12], "sample": None}


def test_large_outputs_are_a_fixed_sample_under_the_budget(tmp_path):
    g = torch.Generator().manual_seed(0)
    outs = {"img": torch.randn(16, 2, 440, 1024, generator=g), "x_start": torch.randn(16, 2, 440, 1024, generator=g)}
    bench.dump_outputs(outs, str(tmp_path / "a"))
    bench.dump_outputs(outs, str(tmp_path / "b"))
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 10 ** 6
    n = outs["img"].numel()
    k = bench.DUMP_BUDGET_BYTES // 4 // 2
    idx = np.sort(np.random.default_rng(bench.DUMP_SEED).choice(n, k, replace=False))
    for name, t in outs.items():
        x, y = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert x.dtype == np.float32 and x.shape == (k,)
        assert np.array_equal(x, y) and np.array_equal(x, t.numpy().reshape(-1)[idx])
