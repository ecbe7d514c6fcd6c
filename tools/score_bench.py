#!/usr/bin/env python3
"""Teacher-forced scoring under the semantic-to-acoustic GPT (csrc/gpt_score.hip): the time of one full-size call against the prefill it
contains plus the head's arithmetic at the fp32 GEMM's known rate (writes profiles/score.txt).

    python tools/score_bench.py [--out-dir profiles] [--rows 64] [--reps 3]

Needs the MI355X (no CPU path: without a device it fails). The full-size model (12 layers, 53376 ids, block 1024) on seeded synthetic weights; --rows rows
of 250 + 1 + 750 seeded ids, scored from position 251 on, at head_rows 256, 1024 and 4096. Every figure is device-event time around one call, which ends in
the product path's own synchronisation (the read of the results), one warm-up, median of --reps runs with the min .. max spread. Beside it, an
``at_gpt_generate`` call with ``max_new = 1`` on the same rows as prompts: the prefill alone, the code generation has always run. The yardstick is that
prefill plus the head's 2 * positions * 768 * 53376 flop at the 139 to 157 TFLOP/s gemm_f32.hip has shown; the file states the ratio of
the yardstick to the time achieved, and what the head's own launches take when they run alone on a chunk. Then, from the GPU tests' own verification
(tests/test_gpt_score_gpu.py: verify), the largest logit and log-prob differences against the float64 twin.
"""
import argparse
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--rows", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, score_logits, seeded_uniforms  # noqa: E402

GEMM_TFLOPS = (139.0, 157.0)   # what gemm_f32.hip has shown on this device
SOURCE, NEW = 250, 750
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


def timed(fn, reps):
    fn()
    t = [once(fn) for _ in range(reps)]
    return statistics.median(t), min(t), max(t)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("score_bench needs the GPU: there is nothing to measure on a CPU")
    cfg = Wav2VecBertDecoderConfig()
    V, E = cfg.VOCAB_SIZE, 768
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    w = W.synth_gpt_weights(n_layer=12, vocab=V, block=1024, seed=0, family="uniform")
    dec = SemanticToAcoustic(cfg, device="cuda:0", weights=w)
    B, L = args.rows, SOURCE + 1 + NEW
    rng = np.random.default_rng(23)
    seqs = [rng.integers(0, V, size=L).astype(np.int32) for _ in range(B)]
    froms = [SOURCE + 1] * B
    positions = B * NEW
    head_tflop = 2.0 * positions * E * V / 1e12
    say(f"tools/score_bench.py on {torch.cuda.get_device_name(0)}: 12 layers, V = {V}, block 1024; {B} rows of {SOURCE} + 1 + {NEW} ids, {positions} scored "
        f"positions; device-event ms, one warm-up, median of {args.reps} [min .. max]")
    u = seeded_uniforms(5, B, 1)
    pre, pre_lo, pre_hi = timed(lambda: dec.generate(seqs, 1, uniforms=u), args.reps)
    say(f"the prefill alone (at_gpt_generate, max_new = 1, the same {B} rows as prompts): {pre:.1f} ms [{pre_lo:.1f} .. {pre_hi:.1f}]")
    lo, hi = (head_tflop / r * 1e3 for r in reversed(GEMM_TFLOPS))
    say(f"the head: {head_tflop:.2f} TFLOP, {lo:.1f} to {hi:.1f} ms at {GEMM_TFLOPS[1]:.0f} to {GEMM_TFLOPS[0]:.0f} TFLOP/s; the yardstick is the prefill plus that: "
        f"{pre + lo:.1f} to {pre + hi:.1f} ms")
    say()
    for head_rows in (256, 1024, 4096):
        med, t_lo, t_hi = timed(lambda: dec.score_rows(seqs, froms, head_rows=head_rows), args.reps)
        say(f"head_rows = {head_rows:4d}: {med:.1f} ms [{t_lo:.1f} .. {t_hi:.1f}] = {positions / med:,.0f} positions/ms; yardstick / achieved = "
            f"{(pre + lo) / med:.2f} to {(pre + hi) / med:.2f}; beyond the prefill {med - pre:.1f} ms, {head_tflop / (med - pre) * 1e3:.0f} TFLOP/s if it were all the head's GEMM")
    say()
    # where the rest goes: the row rule alone on one chunk of logits (two reads of the chunk and its reductions), scaled to the call
    for head_rows in (1024, 4096):
        z = torch.randn((head_rows, V), device="cuda:0")
        t = torch.randint(0, V, (head_rows,), dtype=torch.int32, device="cuda:0")
        med, t_lo, t_hi = timed(lambda: score_logits(z, t, 1.0), args.reps)
        chunks = positions / head_rows
        say(f"the row rule alone on a [{head_rows}][{V}] chunk: {med:.3f} ms [{t_lo:.3f} .. {t_hi:.3f}] = {2 * z.numel() * 4 / med / 1e9:.2f} TB/s over its two reads; "
            f"x {chunks:.1f} chunks = {med * chunks:.1f} ms of the call")
        del z, t
    say()
    # parity, as the GPU tests verify it
    from tests import test_gpt_score_gpu as T
    for family in T.FAMILIES:
        T.test_rows_of_every_length(family)
    T.test_real_vocabulary_through_the_public_interface()
    say(f"parity (tests/test_gpt_score_gpu.py: rows of 2 to 1024 ids on the 2-layer models of both families, and the real vocabulary): largest logit difference "
        f"against the float64 twin {T.RECORD['logit']:.3e} (bar {T.FLOAT_TOL:g}); largest log-prob difference against the twin {T.RECORD['logprob']:.3e}, against "
        f"the rule on the device's own logits {T.RECORD['logprob_on_device_logits']:.3e} (derived bound at least {T.SR.logprob_bound(0):.2e})")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "score.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/score.txt")


if __name__ == "__main__":
    main()
