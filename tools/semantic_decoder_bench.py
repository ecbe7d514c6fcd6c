#!/usr/bin/env python3
"""The semantic-to-acoustic GPT decoder (csrc/gpt.hip): time per generated token against the weight-streaming floor and against the CPU restatement's
uncached loop (writes profiles/semantic_decoder.txt).

    python tools/semantic_decoder_bench.py [--out-dir profiles] [--prompt 251] [--steps 128] [--reps 3] [--cpu-tokens 3]

Needs the MI355X (no CPU path: without a device it fails). The full-size model (12 layers, 53376 ids, block 1024) on seeded synthetic weights; prompts and
draws are seeded. Every figure is device-event time around one ``generate`` call, which ends in the product path's own synchronisation (the read of the
rows' lengths), median of --reps runs with the min .. max spread. A call is the prefill plus its steps, so the time of one step is the difference between a
call of 16 + --steps tokens and a call of 16 tokens, divided by --steps; the two calls alternate. Reported at B = 1, 16 and 64:

  ms per step, tokens/s (B / step time)
  the floor: the bytes of the weights one step streams (12 layers x 7 077 888 parameters + the tied 53376 x 768 head, fp32) at 6.3 TB/s
  the CPU restatement (tests/gpt_ref.py, float32, the whole sequence recomputed per token) on --cpu-tokens tokens of one row

and, from one verified generation (tests/test_semantic_decoder_gpu.py: verify_generation), the largest logit difference against the float64 twin and the
number of waived steps.
"""
import argparse
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--prompt", type=int, default=251)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cpu-tokens", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, seeded_uniforms  # noqa: E402

HBM_TBS = 6.3      # achievable HBM rate of the MI355X
BASE = 16          # tokens of the shorter call
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


def main():
    if not torch.cuda.is_available():
        raise SystemExit("semantic_decoder_bench needs the GPU: there is nothing to measure on a CPU")
    cfg = Wav2VecBertDecoderConfig()
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    w = W.synth_gpt_weights(n_layer=12, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="uniform")
    dec = SemanticToAcoustic(cfg, device="cuda:0", weights=w)
    step_bytes = 4 * (12 * 7077888 + cfg.VOCAB_SIZE * 768)
    floor_ms = step_bytes / (HBM_TBS * 1e12) * 1e3
    say(f"tools/semantic_decoder_bench.py on {torch.cuda.get_device_name(0)}: 12 layers, V = {cfg.VOCAB_SIZE}, block 1024, prompt {args.prompt}, "
        f"step time from calls of {BASE} and {BASE + args.steps} tokens, device-event ms, median of {args.reps} [min .. max]")
    say(f"floor: {step_bytes / 1e6:.1f} MB of fp32 weights per step at {HBM_TBS} TB/s = {floor_ms * 1e3:.1f} us per step, whatever B")
    say()
    rng = np.random.default_rng(11)
    for B in (1, 16, 64):
        prompts = [rng.integers(0, cfg.VOCAB_SIZE, size=args.prompt).astype(np.int32) for _ in range(B)]
        u = seeded_uniforms(5, B, BASE + args.steps)
        short = lambda: dec.generate(prompts, BASE, uniforms=u[:, :BASE])
        long = lambda: dec.generate(prompts, BASE + args.steps, uniforms=u)
        short(), long()
        per_step, calls = [], []
        for _ in range(args.reps):
            a, b = once(short), once(long)
            per_step.append((b - a) / args.steps)
            calls.append(b)
        med = statistics.median(per_step)
        say(f"B = {B:2d}: {med:.4f} ms per step [{min(per_step):.4f} .. {max(per_step):.4f}] = {B / med * 1e3:,.0f} tokens/s; {med / floor_ms:.1f} x the floor; "
            f"a call of {BASE + args.steps} tokens with its prefill {statistics.median(calls):.1f} ms")
    say()
    # the CPU restatement's uncached loop, one row
    from tests import gpt_ref as R
    seq = rng.integers(0, cfg.VOCAB_SIZE, size=args.prompt).astype(np.int64)
    t0 = time.perf_counter()
    for s in range(args.cpu_tokens):
        logits = R.forward(w, seq, torch.float32, positions=[len(seq) - 1])[0].numpy()
        seq = np.append(seq, R.sample(logits, 0.8, 100, 0.5)[0])
    cpu_ms = (time.perf_counter() - t0) * 1e3 / args.cpu_tokens
    say(f"CPU restatement, uncached float32 loop, one row at length {args.prompt}: {cpu_ms:.0f} ms per token over {args.cpu_tokens} tokens "
        f"({torch.get_num_threads()} threads)")
    say()
    # parity of one verified generation, as the GPU tests run it
    from tests import test_semantic_decoder_gpu as T
    for family in ("uniform", "peaky"):
        wf = w if family == "uniform" else W.synth_gpt_weights(n_layer=12, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family=family)
        d = dec if family == "uniform" else SemanticToAcoustic(cfg, device="cuda:0", weights=wf)
        prompts = T.prompts_of([251, 251], cfg.VOCAB_SIZE)
        uu = seeded_uniforms(T.SEED, 2, 32)
        ids, finish, logits = d.generate(prompts, 32, uniforms=uu, return_logits=True)
        worst, waived = T.verify_generation(wf, d, prompts, ids, finish, logits, uu, 0.8, 100, -1, 32)
        say(f"parity, {family} family, B = 2, prompt 251, 32 new tokens: largest logit difference against the float64 twin {worst:.3e} "
            f"(bar {T.FLOAT_TOL:g}); waived steps {waived} of 64")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "semantic_decoder.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/semantic_decoder.txt")


if __name__ == "__main__":
    main()
