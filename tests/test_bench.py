"""bench.py's command line and --dump-outputs writer (CPU only: no device)."""
import os
import sys

import numpy as np
import pytest

from imsame_amd import PARITY_FIELDS, RESULT_DTYPE


@pytest.fixture
def bench():
    """bench.py as a module; as a program it raises GPU_MAX_HW_QUEUES when it
    starts, which must not leak into the tests that run after this one."""
    had = os.environ.get("GPU_MAX_HW_QUEUES")
    import bench as b
    if had is None:
        os.environ.pop("GPU_MAX_HW_QUEUES", None)
    else:
        os.environ["GPU_MAX_HW_QUEUES"] = had
    return b


def _rows(n, seed):
    rng = np.random.default_rng(seed)
    res = np.zeros(n, dtype=RESULT_DTYPE)
    for f in PARITY_FIELDS:
        res[f] = rng.integers(0, 25_000, n)
    res["score"] -= 12_000                       # negative scores survive the cast
    return res


def test_dump_outputs_whole(bench, tmp_path):
    res = _rows(1000, 1)
    bench.dump_outputs(str(tmp_path / "d"), res, 0, 1)
    assert sorted(os.listdir(tmp_path / "d")) == sorted(f + ".npy" for f in PARITY_FIELDS)
    for f in PARITY_FIELDS:
        got = np.load(tmp_path / "d" / (f + ".npy"))
        assert got.dtype == (np.float64 if f in ("db_seq", "score") else np.float32)
        assert np.array_equal(got.astype(np.int64), res[f].astype(np.int64)), f


def test_dump_outputs_sample_is_fixed_and_bounded(bench, tmp_path):
    """Above 1M rows: the same seeded sample for any two runs, with its row
    numbers, and at most 64 MB in all."""
    res = _rows(1_000_001, 2)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), res, 0, 1)
    rows = np.load(tmp_path / "a" / "rows.npy")
    assert rows.dtype == np.float64 and len(rows) == bench.DUMP_MAX_ROWS and np.all(np.diff(rows) > 0)
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))
    idx = rows.astype(np.int64)
    total = 0
    for name in os.listdir(tmp_path / "a"):
        total += os.path.getsize(tmp_path / "a" / name)
        if name != "rows.npy":
            assert np.array_equal(np.load(tmp_path / "a" / name).astype(np.int64),
                                  res[name[:-4]][idx].astype(np.int64)), name
    assert total <= 64_000_000


def test_full_only_legs_need_full(bench, monkeypatch, capsys):
    """A plain run has no CPU baseline, parity or end-to-end leg: asking for
    one without --full is an error, and the defaults parse either way."""
    for argv in (["--e2e", "on"], ["--cpu-sample", "100"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit):
            bench.parse()
        monkeypatch.setattr(sys, "argv", ["bench.py", "--full"] + argv)
        assert bench.parse().full
    capsys.readouterr()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2",
                                      "--dump-outputs", "x"])
    a = bench.parse()
    assert (a.full, a.steps, a.warmup, a.dump_outputs) == (False, 7, 2, "x")
