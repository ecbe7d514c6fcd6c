"""bench.py end to end on the device at small sizes: a plain run prints the contract's line from the timed steps alone (no tapped loop, oracle check,
CPU baseline or extra legs) and --dump-outputs writes the last timed step's codes / token ids, the same on a second run with the same arguments;
--full still adds the rooflines, breakdowns and the oracle check."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--batch", "4", "--seconds", "2", "--sem-batch", "2", "--sem-seconds", "4", "--sem-layers", "2"]


def _bench(args, tmp_path, name):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    detail = str(tmp_path / f"{name}_detail.json")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + args + ["--detail-out", detail],
                       env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0]), json.load(open(detail))


@pytest.mark.gpu
def test_plain_run_and_dumped_outputs(cuda_device, tmp_path):
    runs = []
    for i in range(2):
        line, full = _bench(["--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path / f"out{i}")], tmp_path, f"plain{i}")
        runs.append((line, full))
    line, full = runs[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0 and line["unit"] == "audio-s/s" and line["higher_is_better"] is True
    assert line["metric"] == "audio-sec tokenized / wall-sec (acoustic + semantic_m)"
    assert abs(line["value"] - (4 * 2 + 2 * 4) / (line["ms_per_step"] * 1e-3)) <= 1e-3 * line["value"] + 0.01
    assert line["roofline"] is None and line["cpu_baseline"] is None and "verify" not in line
    for leg in ("semantic_s", "acoustic_decode", "files", "verify"):
        assert leg not in full, leg
    for name in ("acoustic", "semantic_m"):
        assert "breakdown" not in full[name] and "pcie_inclusive" not in full[name]
    dominant = max(("acoustic", "semantic_m"), key=lambda n: full[n]["ms_per_step"])
    assert line["dtype"] == full[dominant]["dtype"]
    for i, (ln, _) in enumerate(runs):
        d = tmp_path / f"out{i}"
        assert sorted(os.listdir(d)) == ["acoustic_codes.npy", "semantic_m_tokens.npy"]
        codes, toks = np.load(d / "acoustic_codes.npy"), np.load(d / "semantic_m_tokens.npy")
        assert codes.dtype == np.float32 and codes.shape == (4, 8, 150) and toks.dtype == np.float32 and toks.shape[:2] == (2, 1)
        assert int(codes.astype(np.int64).sum()) == ln["workloads"]["acoustic"]["token_checksum"]
        assert int(toks.astype(np.int64).sum()) == ln["workloads"]["semantic_m"]["token_checksum"]
    for n in ("acoustic_codes.npy", "semantic_m_tokens.npy"):   # same arguments, same inputs, same outputs
        assert np.array_equal(np.load(tmp_path / "out0" / n), np.load(tmp_path / "out1" / n)), n


@pytest.mark.gpu
def test_full_run_keeps_the_extra_measurements(cuda_device, tmp_path):
    line, full = _bench(["--full", "--workload", "both", "--steps", "2", "--warmup", "1", "--no-cpu-baseline"], tmp_path, "full")
    assert line["steps"] == 2 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] and line["roofline"]["workload"] in ("acoustic", "semantic_m")
    for name in ("acoustic", "semantic_m"):
        assert full[name]["breakdown"] and "roofline" in full[name] and "pcie_inclusive" in full[name]
        assert full["verify"][name]["ids_checked"] > 0
