"""bench.dump_outputs: what --dump-outputs writes (no GPU needed)."""
import os

import numpy as np
import torch


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_dtypes_and_values(tmp_path):
    import bench
    rs = np.random.RandomState(1)
    y = torch.from_numpy(rs.standard_normal((6, 2, 9)).astype(np.float32))
    tgt = torch.nn.functional.one_hot(torch.arange(6) % 2, 2)              # int64
    mix = np.array([3, 0, 5, 1, 4, 2], dtype=np.int64)
    bench.dump_outputs(str(tmp_path), {"data": y, "target": tgt, "mix": mix, "lam": np.float64(0.25)})
    got = _load(tmp_path)
    assert sorted(got) == ["data", "lam", "mix", "target"]
    assert got["data"].dtype == np.float32 and np.array_equal(got["data"], y.numpy())
    assert got["target"].dtype == np.float64 and np.array_equal(got["target"], tgt.numpy())
    assert got["mix"].dtype == np.float64 and np.array_equal(got["mix"], mix)
    assert got["lam"].dtype == np.float64 and got["lam"] == 0.25


def test_dump_outputs_samples_rows_beyond_budget(tmp_path):
    import bench
    B, C, T = 64, 2, 100
    y = np.arange(B * C * T, dtype=np.float32).reshape(B, C, T)
    mix = np.arange(B)[::-1].copy()
    budget = 20 * C * T * 4
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"data": y, "mix": mix, "empty": []}, budget=budget)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert sorted(a) == ["data", "empty", "mix", "rows"]
    assert sum(v.nbytes for v in a.values()) <= budget
    rows = a["rows"].astype(np.int64)
    assert 0 < len(rows) < B and np.all(np.diff(rows) > 0)
    assert np.array_equal(a["data"], y[rows]) and np.array_equal(a["mix"], mix[rows])
    assert a["empty"].shape == (0,)
    for k in a:                                                          # the same sample every run
        assert np.array_equal(a[k], b[k])
