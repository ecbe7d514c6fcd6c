#!/usr/bin/env python3
"""The fine stage (csrc/fine.hip): time per window against the fp32 GEMM's floor and against ``transformers``' ``BarkFineModel.generate`` on the host CPU
(writes profiles/fine_decoder.txt).

    python tools/fine_decoder_bench.py [--out-dir profiles] [--reps 3] [--cpu-threads 16] [--no-cpu]

Needs the MI355X (no CPU path: without a device it fails). Two seeded synthetic models at W = 1024: 12 layers / 768 and 24 layers / 1024, no linear biases.
A window is six forwards (code books 2 to 7) over B x 1024 positions plus six sampling launches. Every figure is device-event time around one ``generate``
call of B rows of T = 1024 frames (one window, every position predicted), which ends in the product path's own synchronisation (the copy of the codes);
one warm-up call, then the median of --reps calls with the min .. max spread. Reported at B = 1, 16 and 64:

  ms per window, frames/s = B * 512 / window time: in a long row every window but the last adds W / 2 = 512 new frames
  the floor of this design: the window's matrix-product FLOPs (four linears per block and the 1024-column head, 2 M N K each) at the 139 TFLOP/s the fp32
  matrix-core GEMM reaches on the conformer's FFN shape (csrc/gemm_f32.hip); the attention's 4 W^2 E FLOPs per layer and window are listed beside it
  HF's ``BarkFineModel.generate`` (float32, argmax path) on this host's CPU with --cpu-threads threads for one row of the same T

and, from verified generations as the GPU tests run them (tests/test_fine_decoder_gpu.py: verify), the largest logit difference against the float64 twin
and the number of waived draws.
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu-threads", type=int, default=16)
ap.add_argument("--no-cpu", action="store_true")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.fine_decoder import CoarseToFine, seeded_uniforms  # noqa: E402

GEMM_TFLOPS = 139.0    # launch_gemm on the conformer's ffn2 shape (csrc/gemm_f32.hip)
BLOCK = 1024
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def window_flops(n_layer, E, B):
    rows = B * BLOCK
    gemm = 6 * (n_layer * 2 * rows * 12 * E * E + 2 * rows * 1024 * E)
    attn = 6 * n_layer * B * 4 * BLOCK * BLOCK * E
    return gemm, attn


def hf_window_seconds(w, n_layer, E, threads):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_fine as G
    torch.set_num_threads(threads)
    model = G.hf_model(w, BLOCK, n_layer, E, False)
    coarse = np.random.default_rng(3).integers(0, 1024, size=(2, BLOCK))
    t0 = time.perf_counter()
    G.hf_generate(model, coarse, BLOCK)
    return time.perf_counter() - t0


def main():
    if not torch.cuda.is_available():
        raise SystemExit("fine_decoder_bench needs the GPU: there is nothing to measure on a CPU")
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    say(f"tools/fine_decoder_bench.py on {torch.cuda.get_device_name(0)}: W = {BLOCK}, one window = 6 forwards + 6 sampling launches over B x {BLOCK} positions, "
        f"temperature 0.5, device-event ms around one generate call of T = {BLOCK}, one warm-up, median of {args.reps} [min .. max]")
    say(f"floor: the window's GEMM FLOPs at {GEMM_TFLOPS:.0f} TFLOP/s (fp32 matrix-core GEMM, csrc/gemm_f32.hip); launches per forward: 7 per layer + 3 "
        f"(embedding, final LayerNorm, head; + 1 gather where a window has rel > 0), + 1 sampling launch")
    rng = np.random.default_rng(11)
    for n_layer, E in ((12, 768), (24, 1024)):
        w = W.synth_fine_weights(n_layer, E, BLOCK, seed=0, family="uniform")
        dec = CoarseToFine(device="cuda:0", weights=w)
        say()
        say(f"{n_layer} layers / {E}: {7 * n_layer + 4} launches per forward and its sampling, {6 * (7 * n_layer + 4) + 2} per one-window call")
        for B in (1, 16, 64):
            rows = [rng.integers(0, 1024, size=(2, BLOCK)) for _ in range(B)]
            u = seeded_uniforms(5, B, 1, BLOCK)
            call = lambda: dec.generate(rows, temperature=0.5, uniforms=u)
            call()
            ms = [once(call) for _ in range(args.reps)]
            med = statistics.median(ms)
            gemm, attn = window_flops(n_layer, E, B)
            floor = gemm / (GEMM_TFLOPS * 1e12) * 1e3
            say(f"  B = {B:2d}: {med:9.2f} ms per window [{min(ms):.2f} .. {max(ms):.2f}] = {B * 512 / med * 1e3:10,.0f} frames/s; GEMM {gemm / 1e12:7.2f} TFLOP "
                f"(+ attention {attn / 1e12:.2f}) -> floor {floor:8.2f} ms, {med / floor:.2f} x the floor; {gemm / med / 1e9:.1f} TFLOP/s of GEMM work sustained")
        del dec
        torch.cuda.empty_cache()
        if not args.no_cpu:
            sec = hf_window_seconds(w, n_layer, E, args.cpu_threads)
            say(f"  HF BarkFineModel.generate, float32, argmax path, one row of T = {BLOCK} on the host CPU ({torch.get_num_threads()} threads): {sec * 1e3:,.0f} ms "
                f"per window = {512 / sec:,.0f} frames/s")
    say()
    # parity of verified generations, as the GPU tests run them
    from tests import fine_cases as K
    from tests import test_fine_decoder_gpu as T
    for m in ("a", "b"):
        for family in K.FAMILIES:
            Wd = K.MODELS[m]["block"]
            before = dict(T.RECORD)
            T.run(m, family, [1, Wd, Wd + 1, 2 * Wd + 3])
            say(f"parity, model {m} ({K.MODELS[m]['n_layer']} layers / {K.MODELS[m]['hidden']}, W = {Wd}), {family} family, rows [1, W, W + 1, 2 W + 3] in one call: "
                f"waived {T.RECORD['waived'] - before['waived']} of {T.RECORD['draws'] - before['draws']} draws (window {T.R.WINDOW:.2e}, cap 2 %)")
    T.test_real_size_window()
    say(f"largest logit difference against the float64 twin over these and the real-size case (W = 1024, T = 1025): {T.RECORD['max_logit_diff']:.3e} "
        f"(bar {T.FLOAT_TOL:g}); waived {T.RECORD['waived']} of {T.RECORD['draws']} draws in all")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "fine_decoder.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/fine_decoder.txt")


if __name__ == "__main__":
    main()
