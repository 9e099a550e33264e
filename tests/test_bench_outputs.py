"""bench.py --dump-outputs on the host: file names, dtypes, the seeded sample of a large array and the size limit.  CPU only."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_writes_float32_and_float64_arrays_by_name(tmp_path):
    small = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    table = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    bench.dump_outputs({"params.dense.kernel": small, "ber_table": table, "conf": np.eye(2)}, str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["ber_table.npy", "conf.npy", "params.dense.kernel.npy"]
    a = np.load(tmp_path / "out" / "params.dense.kernel.npy")
    assert a.dtype == np.float32 and a.shape == (3, 4) and np.array_equal(a, small.numpy())
    t = np.load(tmp_path / "out" / "ber_table.npy")
    assert t.dtype == np.float64 and np.array_equal(t, table.numpy())
    assert np.load(tmp_path / "out" / "conf.npy").dtype == np.float64


def test_dump_of_a_large_array_is_the_same_seeded_sample_every_time(tmp_path):
    n = bench.DUMP_CAP * 3 + 7
    big = torch.arange(n, dtype=torch.float32)
    bench.dump_outputs({"big": big}, str(tmp_path / "a"))
    bench.dump_outputs({"big": big * 1.0}, str(tmp_path / "b"))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.shape == (bench.DUMP_CAP,) and a.dtype == np.float32 and np.array_equal(a, b)
    # the sample is the array's own elements at sorted indices spread over the whole array
    assert np.all(np.diff(a) >= 0) and a[0] < n / 100 and a[-1] > n * 0.99 and np.all(a == np.round(a))


def test_dump_refuses_more_than_the_size_limit(tmp_path):
    arrays = {"a%d" % i: torch.zeros(bench.DUMP_CAP, dtype=torch.float64) for i in range(bench.DUMP_LIMIT // (8 * bench.DUMP_CAP) + 1)}
    with pytest.raises(SystemExit):
        bench.dump_outputs(arrays, str(tmp_path / "out"))
    assert not os.path.exists(tmp_path / "out") or not os.listdir(tmp_path / "out")
