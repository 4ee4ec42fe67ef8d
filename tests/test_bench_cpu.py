"""bench.py --dump-outputs writer (host side only): float32 values, float64 ids, a fixed seeded sample of a large array."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dump_outputs_dtypes_and_sample(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    ids = np.array([3, 31999], np.int32)
    vals = np.array([[0.5, -1.25]], np.float16)
    big = np.arange(bench.DUMP_MAX_ELEMS + 1000, dtype=np.float64).reshape(-1, 8)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), dict(token_ids=ids, logits=vals, big=big))
    got_ids = np.load(tmp_path / "a" / "token_ids.npy")
    assert got_ids.dtype == np.float64 and np.array_equal(got_ids, ids)
    got_vals = np.load(tmp_path / "a" / "logits.npy")
    assert got_vals.dtype == np.float32 and np.array_equal(got_vals, vals.astype(np.float32))
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.size == bench.DUMP_MAX_ELEMS and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and np.isin(a, big.astype(np.float32).ravel()).all()
