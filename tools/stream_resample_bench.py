#!/usr/bin/env python3
"""The streaming resampler against what it follows (writes profiles/stream_resample.txt).

    python tools/stream_resample_bench.py [--out-dir profiles] [--rows 64] [--seconds 10] [--files 64] [--file-seconds 60] [--chunk-size 10]
                                          [--reps 5] [--launches 20] [--file-reps 3]

Needs the MI355X (no CPU path: without a device it fails). Two comparisons, each inside one run, the two sides alternating, after a warm-up of both:

  (a) at_resample_rows against at_segments_from_pcm on the same --rows x --seconds of 44.1 kHz int16 PCM resident on the device, every row the whole
      signal (one chunk / one final row), no mask: device events around --launches back-to-back launches, --reps repeats, median and min .. max. The two
      outputs are compared first (they must be equal, bit for bit).
  (b) files to tokens: encode_batch_files(stream=True) with resample="file" against resample="chunk" on --files 44.1 kHz int16 WAV files of
      --file-seconds each (seeded, written to a temporary directory), batch_size = --files, synthetic weights, K = 8: wall clock around the whole call
      (it ends with the tokens on disk), --file-reps repeats, audio seconds per second.
"""
import argparse
import ctypes as C
import os
import shutil
import statistics
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--seconds", type=int, default=10)
ap.add_argument("--files", type=int, default=64)
ap.add_argument("--file-seconds", type=int, default=60)
ap.add_argument("--chunk-size", type=int, default=10)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--launches", type=int, default=20)
ap.add_argument("--file-reps", type=int, default=3)
ap.add_argument("--num-workers", type=int, default=8)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import AudioToken, Tokenizers, _cabi  # noqa: E402
from audiotoken_amd import resample_stream as RS  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.writer import WavWriter  # noqa: E402

assert torch.cuda.is_available(), "tools/stream_resample_bench.py measures on the device: no HIP device found"
DEV, RATE, MODEL = "cuda:0", 44100, 24000
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def spread(xs):
    return f"{statistics.median(xs):.4g} ({min(xs):.4g} .. {max(xs):.4g})"


def pcm_rows(rows, samples, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    t = torch.arange(samples, device=DEV, dtype=torch.float32) / RATE
    x = 0.3 * torch.sin(2 * torch.pi * 440.0 * t)[None] + 0.3 * (torch.rand((rows, samples), device=DEV, generator=g) * 2 - 1)
    return torch.round(x * 32767.0).to(torch.int16).contiguous()


def kernel_comparison():
    lib = _cabi.load()
    rs = RS.DeviceResampler(DEV, MODEL)
    R, L = args.rows, args.seconds * RATE
    pcm = pcm_rows(R, L, 1)
    tptr, o, n, width = rs.table(RATE)
    Lr = RS.ceil_div(n * L, o)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    segs = (_cabi.SegmentDesc * R)(*[_cabi.SegmentDesc(pcm[r].data_ptr(), tptr, 0, L, 0, Lr, _cabi.PCM_S16, 1.0 / 32768.0, o, n, width, Lr) for r in range(R)])
    plan = RS.PushPlan(0, Lr, 0, L, L, True, 0, 0)
    rows = (_cabi.ResampleRow * R)(*[_cabi.ResampleRow(*plan.row(pcm[r].data_ptr(), tptr, _cabi.PCM_S16, 1.0 / 32768.0, o, n, width, r * Lr)) for r in range(R)])
    _cabi.check(lib.at_resample_rows_check(C.addressof(rows), R), "at_resample_rows_check")
    d_segs = torch.from_numpy(np.frombuffer(segs, dtype=np.uint8).copy()).to(DEV)
    d_rows = torch.from_numpy(np.frombuffer(rows, dtype=np.uint8).copy()).to(DEV)
    out_a = torch.empty((R, Lr), dtype=torch.float32, device=DEV)
    out_b = torch.empty((R, Lr), dtype=torch.float32, device=DEV)

    def feeder():
        _cabi.check(lib.at_segments_from_pcm(d_segs.data_ptr(), R, Lr, 0.0, out_a.data_ptr(), None, stream), "at_segments_from_pcm")

    def streamed():
        _cabi.check(lib.at_resample_rows(d_rows.data_ptr(), R, out_b.data_ptr(), stream), "at_resample_rows")

    for _ in range(3):
        feeder()
        streamed()
    torch.cuda.synchronize()
    same = bool(torch.equal(out_a, out_b))
    times = {"at_segments_from_pcm": [], "at_resample_rows": []}
    for rep in range(args.reps):
        for name, fn in (("at_segments_from_pcm", feeder), ("at_resample_rows", streamed))[::1 if rep % 2 == 0 else -1]:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                fn()
            b.record()
            b.synchronize()
            times[name].append(a.elapsed_time(b) / args.launches)
    say(f"(a) {R} rows x {args.seconds} s of 44.1 kHz int16 -> {R} x {Lr} float32 at 24 kHz, every row the whole signal; ms per launch, median (min .. max) of "
        f"{args.reps} repeats of {args.launches} launches, the two alternating; outputs equal bit for bit: {same}")
    out_bytes = R * Lr * 4 + R * L * 2
    for name, ts in times.items():
        say(f"    {name:22s} {spread(ts)} ms    {out_bytes / statistics.median(ts) / 1e6:.0f} GB/s of samples read once + written once")
    ratio = statistics.median(times["at_resample_rows"]) / statistics.median(times["at_segments_from_pcm"])
    say(f"    at_resample_rows / at_segments_from_pcm = {ratio:.3f}")
    assert same, "the two kernels disagree"


def write_files(root):
    rng = np.random.default_rng(7)
    n = args.file_seconds * RATE
    t = np.arange(n, dtype=np.float64) / RATE
    for i in range(args.files):
        x = 0.3 * np.sin(2 * np.pi * (200.0 + 10 * i) * t) + 0.3 * rng.uniform(-1.0, 1.0, n)
        w = WavWriter(os.path.join(root, f"f{i:03d}.wav"), RATE)
        w.write(np.round(x * 32767.0).astype(np.int16))
        w.close()


def files_comparison():
    tok = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8, weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    root = tempfile.mkdtemp(prefix="stream_resample_bench_")
    try:
        src = os.path.join(root, "audio")
        os.makedirs(src)
        write_files(src)
        audio_s = args.files * args.file_seconds

        def run(mode, tag):
            out = os.path.join(root, f"tokens_{mode}_{tag}")
            t0 = time.perf_counter()
            tok.encode_batch_files(batch_size=args.files, outdir=out, chunk_size=args.chunk_size, num_workers=args.num_workers, audio_dir=src, stream=True,
                                   resample=mode)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert tok.skipped_files == [] and len(os.listdir(out)) == args.files
            shutil.rmtree(out)
            return dt
        run("file", "warm")
        run("chunk", "warm")
        times = {"file": [], "chunk": []}
        for rep in range(args.file_reps):
            for mode in ("file", "chunk")[::1 if rep % 2 == 0 else -1]:
                times[mode].append(run(mode, str(rep)))
        say(f"(b) {args.files} files x {args.file_seconds} s of 44.1 kHz int16 WAV -> token files, encode_batch_files(stream=True, batch_size={args.files}, "
            f"chunk_size={args.chunk_size}, num_workers={args.num_workers}), K = 8, synthetic weights; wall clock of the whole call, median (min .. max) of "
            f"{args.file_reps} repeats after one warm-up each, the two alternating")
        for mode, ts in times.items():
            rates = [audio_s / t for t in ts]
            say(f"    resample={mode!r:8s} {spread(ts)} s    {spread(rates)} audio-s/s")
        say(f"    'file' / 'chunk' rate = {statistics.median(times['chunk']) / statistics.median(times['file']):.2f}")
    finally:
        shutil.rmtree(root, ignore_errors=True)


say(f"tools/stream_resample_bench.py on {torch.cuda.get_device_name(0)}")
say()
kernel_comparison()
say()
files_comparison()
if args.out_dir:
    os.makedirs(args.out_dir, exist_ok=True)
    with open(os.path.join(args.out_dir, "stream_resample.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
