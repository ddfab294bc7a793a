"""bench.py --dump-outputs: dump_outputs writes float32 / float64 .npy files that hold every source
value exactly, keeps the directory under its 64 MB cap by a fixed sample of rows, and is the same
from run to run. Host only (numpy arrays in, files out)."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_keeps_values_and_dtypes(tmp_path):
    b = _bench()
    rng = np.random.default_rng(1)
    arrays = {"f32": rng.standard_normal((33, 7)).astype(np.float32), "f64": rng.standard_normal((7, 5)),
              "i8": rng.integers(-1, 3, 19).astype(np.int8), "i32": np.array([2**31 - 1, -2**31], np.int32),
              "i64": np.array([2**40 + 1, -3], np.int64), "u8": np.arange(4, dtype=np.uint8), "scalar": np.float32(1.5)}
    listing = b.dump_outputs(str(tmp_path / "d"), arrays)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(k + ".npy" for k in arrays)
    for k, a in arrays.items():
        got = np.load(tmp_path / "d" / (k + ".npy"))
        assert got.dtype == (np.float64 if k in ("f64", "i32", "i64") else np.float32), k
        assert np.array_equal(got, np.atleast_1d(a)), k  # exact: nothing is rounded on the way out
        assert listing[k][2] == listing[k][3] == got.shape[0]


def test_dump_samples_large_arrays_under_the_cap(tmp_path, monkeypatch):
    b = _bench()
    monkeypatch.setattr(b, "DUMP_CAP_BYTES", 64 * 1024)
    big = np.arange(5000 * 16, dtype=np.float32).reshape(5000, 16)
    arrays = {"big": big, "small": np.ones(3, np.float32)}
    one = b.dump_outputs(str(tmp_path / "a"), arrays)
    two = b.dump_outputs(str(tmp_path / "b"), arrays)
    assert one == two
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 * 1024
    got = np.load(tmp_path / "a" / "big.npy")
    assert 1 < got.shape[0] < 5000 and got.shape[1:] == (16,) and one["big"][2:] == [got.shape[0], 5000]
    rows = (got[:, 0] / 16).astype(int)
    assert np.all(np.diff(rows) > 0) and np.array_equal(got, big[rows])  # whole rows of the source, ascending
    assert np.array_equal(got, np.load(tmp_path / "b" / "big.npy"))  # the same sample on every run
    assert np.array_equal(np.load(tmp_path / "a" / "small.npy"), arrays["small"])
