"""bench.py's run options without a device: --full is off by default, --steps must be at least 1, and --dump-outputs writes the timed path's
arrays as float32 .npy files — whole when they fit, as a fixed seeded sample (with its flat indices) when they exceed the size limit."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_plain_run_is_the_default():
    import bench
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and a.steps == 7 and a.warmup == 2
    assert bench.parse_args(["--full", "--dump-outputs", "d"]).full is True


@pytest.mark.parametrize("argv", [["--steps", "0"], ["--workload", "selftest", "--dump-outputs", "d"], ["--workload", "files", "--dump-outputs", "d"]])
def test_invalid_options_are_refused(argv):
    import bench
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_writes_float32_whole(tmp_path):
    import bench
    codes = torch.arange(2 * 8 * 5, dtype=torch.int16).reshape(2, 8, 5)
    toks = torch.tensor([[0, 2047, 5]], dtype=torch.int16)
    bench.dump_outputs(str(tmp_path / "d"), {"acoustic_codes": codes, "semantic_m_tokens": toks})
    a = np.load(tmp_path / "d" / "acoustic_codes.npy")
    t = np.load(tmp_path / "d" / "semantic_m_tokens.npy")
    assert a.dtype == np.float32 and a.shape == (2, 8, 5) and np.array_equal(a, codes.numpy().astype(np.float32))
    assert t.dtype == np.float32 and t.tolist() == [[0.0, 2047.0, 5.0]]
    assert sorted(os.listdir(tmp_path / "d")) == ["acoustic_codes.npy", "semantic_m_tokens.npy"]


def test_dump_outputs_samples_above_the_limit(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT", 12_000)
    x = torch.arange(10_000, dtype=torch.float32).reshape(100, 100)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"audio": x})
    v, i = np.load(tmp_path / "a" / "audio.npy"), np.load(tmp_path / "a" / "audio_index.npy")
    assert v.dtype == np.float32 and i.dtype == np.float64 and v.shape == i.shape == (1000,)
    assert np.all(np.diff(i) > 0) and np.array_equal(v, x.numpy().reshape(-1)[i.astype(np.int64)])
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= 12_000 + 2 * 128   # + two .npy headers
    assert np.array_equal(v, np.load(tmp_path / "b" / "audio.npy")) and np.array_equal(i, np.load(tmp_path / "b" / "audio_index.npy"))
