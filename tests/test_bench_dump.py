"""`bench.py --dump-outputs`: what it writes, without a GPU (the writer takes any tensor)."""
import numpy as np
import torch

import bench


def test_dump_writes_small_outputs_whole_and_samples_large_ones_the_same_way_every_time(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 4 * 1000)
    small = torch.arange(24, dtype=torch.float32).reshape(1, 2, 3, 4).permute(0, 3, 1, 2)  # a permuted view, like the BEV map
    large = torch.randn(1, 8, 50, 50, dtype=torch.float64)
    for run in ("a", "b"):
        bench.dump_outputs(str(tmp_path / run), {"small": small, "large": large})
    got = np.load(tmp_path / "a" / "small.npy")
    assert got.dtype == np.float32 and got.shape == (1, 4, 2, 3) and np.array_equal(got, small.numpy())
    sample = np.load(tmp_path / "a" / "large.npy")
    assert sample.dtype == np.float32 and sample.shape == (500,)  # half of the 4000-byte budget for each of the two outputs
    assert np.isin(sample, large.float().numpy().reshape(-1)).all()
    assert np.array_equal(sample, np.load(tmp_path / "b" / "large.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 4 * 1000 + 2 * 128  # (+ the .npy headers)
