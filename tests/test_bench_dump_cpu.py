"""bench.py --dump-outputs on the host side: one DIR/<name>.npy per array in float64 (float32 for float32 results) with its
shape, an array of more than DUMP_SAMPLE elements as a sample at fixed seeded positions, and the 64 MB budget."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_every_array_as_float_with_its_shape(tmp_path):
    bench.dump_outputs(str(tmp_path), [("param_w", torch.arange(6, dtype=torch.float64).reshape(2, 3)),
                                       ("scalar_elbo", torch.tensor(-1.5, dtype=torch.float64)),
                                       ("v", torch.ones(4, dtype=torch.float32)),
                                       ("ids", torch.arange(3))])
    assert sorted(os.listdir(tmp_path)) == ["ids.npy", "param_w.npy", "scalar_elbo.npy", "v.npy"]
    w = np.load(tmp_path / "param_w.npy")
    assert w.dtype == np.float64 and np.array_equal(w, np.arange(6.0).reshape(2, 3))
    e = np.load(tmp_path / "scalar_elbo.npy")
    assert e.dtype == np.float64 and e.shape == () and float(e) == -1.5
    assert np.load(tmp_path / "v.npy").dtype == np.float32
    assert np.load(tmp_path / "ids.npy").dtype == np.float64


def test_step_arrays_names_parameters_gradients_and_scalars():
    names = [n for n, _ in bench.step_arrays({"w": torch.zeros(2)}, {"w": torch.ones(2)}, {"elbo": -3.0})]
    assert names == ["param_w", "grad_w", "scalar_elbo"]


def test_dump_samples_a_large_array_at_the_same_positions_every_time(tmp_path):
    n = bench.DUMP_SAMPLE + 12345
    t = torch.arange(n, dtype=torch.float32)            # value = position
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("K_nm", t)])
    a, b = np.load(tmp_path / "a" / "K_nm_sample.npy"), np.load(tmp_path / "b" / "K_nm_sample.npy")
    assert not (tmp_path / "a" / "K_nm.npy").exists()
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert np.all(np.diff(a) >= 0) and 0 <= a.min() and a.max() < n


def test_dump_refuses_more_than_64_MB(tmp_path):
    big = torch.zeros(bench.DUMP_SAMPLE, dtype=torch.float64)          # 8 MB each
    with pytest.raises(SystemExit, match="budget"):
        bench.dump_outputs(str(tmp_path), [(f"a{i}", big) for i in range(9)])
    assert os.listdir(tmp_path) == []
