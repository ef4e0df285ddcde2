"""bench.py's command line: --dump-outputs writes float arrays (a fixed seeded sample of a
large one), and a plain run is the default while --full is an option."""
import sys

import numpy as np
import torch


def test_dump_outputs_sample_is_fixed_and_float(tmp_path):
    import bench
    n = 5 * (bench.DUMP_MAX_ELEMS // 5 + 2469)
    big = torch.arange(n, dtype=torch.float32).reshape(n // 5, 5).to(torch.bfloat16)
    arrays = {"loss": torch.tensor(1.25, dtype=torch.float64), "idx": torch.arange(7, dtype=torch.int64), "big": big}
    info = bench.dump_outputs(str(tmp_path / "a"), arrays)
    bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert info["big"] == {"shape": [n // 5, 5], "written": bench.DUMP_MAX_ELEMS}
    loss, idx = np.load(tmp_path / "a" / "loss.npy"), np.load(tmp_path / "a" / "idx.npy")
    assert loss.dtype == np.float64 and loss.shape == () and loss == 1.25
    assert idx.dtype == np.float32 and idx.tolist() == list(range(7))
    a, pos = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "a" / "big_positions.npy")
    assert a.dtype == np.float32 and pos.dtype == np.float64 and a.shape == pos.shape == (bench.DUMP_MAX_ELEMS,)
    assert (np.diff(pos) >= 0).all() and 0 <= pos[0] and pos[-1] < n
    np.testing.assert_array_equal(a, big.reshape(-1)[torch.from_numpy(pos.astype(np.int64))].float().numpy())
    for f in ("big.npy", "big_positions.npy"):      # same shape, same positions, same sample
        np.testing.assert_array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
    # both tensors a step returns (pred, mask index) sampled, values + positions: below the 64 MB a dump may hold
    assert 2 * bench.DUMP_MAX_ELEMS * (4 + 8) + 4096 < 64e6


def test_plain_is_default_and_full_is_an_option(monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, "", 7, 3)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
