"""bench.py's command line and output writer, without a GPU: --full / --dump-outputs exist, and the dump keeps to its size limit
with a fixed, seeded sample of an array that does not fit."""
import importlib.util
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_help_lists_full_and_dump_outputs():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


def test_write_outputs_keeps_small_arrays_whole(tmp_path):
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)
    _bench().write_outputs(str(tmp_path), {"a": a, "b": np.ones(3, dtype=np.float16)})
    got = np.load(tmp_path / "a.npy")
    assert got.dtype == np.float32 and got.shape == (2, 3, 4) and np.array_equal(got, a)
    assert np.load(tmp_path / "b.npy").dtype == np.float32


def test_write_outputs_samples_what_exceeds_the_limit(tmp_path):
    rng = np.random.default_rng(1)
    big, small = rng.random((50, 1000)), rng.random(100)
    b = _bench()
    for d in (tmp_path / "x", tmp_path / "y"):
        b.write_outputs(str(d), {"big": big, "small": small}, limit=100_000)
    names = sorted(os.listdir(tmp_path / "x"))
    assert names == ["big_sample.npy", "big_sample_index.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "x" / f) for f in names) <= 100_000
    idx = np.load(tmp_path / "x" / "big_sample_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    vals = np.load(tmp_path / "x" / "big_sample.npy")
    assert np.array_equal(vals, big.astype(np.float32).reshape(-1)[idx.astype(np.int64)])
    for f in names:                                   # the sample is seeded: the same on every run
        assert np.array_equal(np.load(tmp_path / "x" / f), np.load(tmp_path / "y" / f))
