"""``bench.py`` without a GPU: its options and what ``--dump-outputs`` writes (``dump_outputs``)."""

import os
import subprocess
import sys

import numpy as np

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402  (numpy only at import: torch and the engine are imported inside main)


def test_help_lists_the_plain_run_options():
    out = subprocess.run([sys.executable, "bench.py", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    for opt in ("--gpus", "--steps", "--warmup", "--full", "--dump-outputs"):
        assert opt in out.stdout


def test_dump_writes_W_and_H_as_float64(tmp_path):
    rng = np.random.default_rng(0)
    W, H = rng.random((50, 96)), rng.random((1000, 50))
    assert bench.dump_outputs(str(tmp_path / "d"), W, H) == ["H", "W"]
    assert sorted(os.listdir(tmp_path / "d")) == ["H.npy", "W.npy"]  # (outside the repository: no .gitignore of its own)
    for name, a in (("W", W), ("H", H)):
        b = np.load(tmp_path / "d" / f"{name}.npy")
        assert b.dtype == np.float64 and np.array_equal(a, b)


def test_dump_of_a_large_H_is_a_fixed_sample_of_its_rows_within_the_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    rng = np.random.default_rng(1)
    W, H = rng.random((50, 96)), rng.random((20000, 50))
    names = bench.dump_outputs(str(tmp_path / "a"), W, H)
    assert names == ["H_rows_sample", "H_rows_sample_index", "W"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 1 << 20
    idx = np.load(tmp_path / "a" / "H_rows_sample_index.npy")
    rows = np.load(tmp_path / "a" / "H_rows_sample.npy")
    assert idx.dtype == rows.dtype == np.float64 and np.all(np.diff(idx) > 0) and len(idx) > 1000
    assert np.array_equal(rows, H[idx.astype(np.int64)])
    bench.dump_outputs(str(tmp_path / "b"), W, H)  # the same rows every time
    assert np.array_equal(idx, np.load(tmp_path / "b" / "H_rows_sample_index.npy"))
