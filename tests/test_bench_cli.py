"""bench.py's host side without a GPU: the --dump-outputs writer and the --steps / --warmup check."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_budget_dtypes_and_fixed_sample(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    g = torch.Generator().manual_seed(0)
    arrays = {"small": torch.randn(4, 18, 8, generator=g), "f64": torch.randn(3, 5, generator=g, dtype=torch.float64),
              "half": torch.randn(2, 3, generator=g).to(torch.bfloat16), "big": torch.randn(8, 3, 128, 128, generator=g),
              "bigger": torch.randn(8, 3, 256, 256, generator=g)}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == sorted(n + ".npy" for n in arrays)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= bench.DUMP_BYTES
    load = lambda d, n: np.load(tmp_path / d / (n + ".npy"))  # noqa: E731
    np.testing.assert_array_equal(load("a", "small"), arrays["small"].numpy())          # fits: written whole, shape kept
    assert load("a", "f64").dtype == np.float64 and load("a", "half").dtype == np.float32
    np.testing.assert_array_equal(load("a", "half"), arrays["half"].float().numpy())
    for n in ("big", "bigger"):                                                            # too large: a sample of the elements
        s = load("a", n)
        assert s.ndim == 1 and 0 < s.size < arrays[n].numel()
        assert np.isin(s, arrays[n].numpy().ravel()).all()
        np.testing.assert_array_equal(s, load("b", n))                                    # the same sample every run


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode != 0 and "--steps must be >= 1" in p.stderr
