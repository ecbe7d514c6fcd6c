"""Measure voice prompts and write profiles/voice_prompt.txt, by the protocol of profiles/long_form.txt: one warm-up, the median of
``--reps`` runs and their spread (max - min).

Part 1: 64 sources of 1500 semantic ids through ``to_audio(long_form=True, slots=64)`` on the full-size 12-layer synthetic GPT at the product geometry
(S = 250, H = 124), the default synthetic fine model and acoustic decoder: unprompted, and with one 126-id prompt (189 frames) shared by all 64.
Part 2: the unprompted leg of tools/long_form_bench.py at B = 16 (``to_acoustic_long`` on 16 such sources) on this build, beside the same leg measured on
the parent commit's build on the same machine (``python tools/long_form_bench.py --batches 16`` there; pass its figures with ``--parent-ms`` /
``--parent-spread-ms``). The prompt-free path should be no slower than the parent beyond the spread profiles/long_form.txt records for that leg.

    python tools/voice_prompt_bench.py [--reps 3] [--sources 64] [--parent-ms X --parent-spread-ms Y]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from long_form_bench import H, MAX_NEW, N_SOURCE, S, plan, r, timed  # noqa: E402

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.voice import VoicePrompt  # noqa: E402


def recorded_b16_spread_ms(path=os.path.join(ROOT, "profiles", "long_form.txt")):
    """The spread profiles/long_form.txt records for its B = 16 device-driven leg."""
    import re
    with open(path) as f:
        for line in f:
            m = re.match(r"B=16: device-driven +[0-9.]+ ms \(spread ([0-9.]+) ms\)", line)
            if m:
                return float(m.group(1))
    raise SystemExit(f"{path} has no B=16 line")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sources", type=int, default=64)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--parent-ms", type=float, default=None)
    ap.add_argument("--parent-spread-ms", type=float, default=None)
    ap.add_argument("--recorded-spread-ms", type=float, default=None, help="default: the B=16 spread in profiles/long_form.txt")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voice_prompt.txt"))
    args = ap.parse_args()
    cfg = Wav2VecBertDecoderConfig()
    gpt = W.synth_gpt_weights(n_layer=args.layers, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device="cuda:0", decoder_weights=gpt)
    rng = np.random.default_rng(0)
    n = args.sources
    srcs = [rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=N_SOURCE).astype(np.int64) for _ in range(max(n, 16))]
    P = S - H
    voice = VoicePrompt(rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=P), rng.integers(0, 1024, size=(8, 3 * P // 2)))
    lines = [f"voice prompts: {n} sources of {N_SOURCE} ids through to_audio(long_form=True, slots={min(n, 64)}), {args.layers}-layer synthetic GPT (vocab "
             f"{cfg.VOCAB_SIZE}, block 1024), S={S} H={H}, max_new_tokens={MAX_NEW}, the default synthetic fine model and acoustic decoder; one warm-up, "
             f"{args.reps} runs each (median, spread = max - min)"]
    kw = dict(long_form=True, window=S, hop=H, max_new_tokens=MAX_NEW, slots=min(n, 64), seed=1)
    for name, v in (("unprompted", None), (f"one shared prompt of {P} ids ({3 * P // 2} frames)", voice)):
        call = lambda: sem.to_audio(srcs[:n], voice=v, **kw)   # noqa: E731
        call()
        (audio, coarse, fine), ms, spread = timed(call, args.reps)
        frames = sum(int(c.shape[1]) for c in fine.codes)
        stage = {}
        for what, fn in (("to_acoustic", lambda: sem.to_acoustic(srcs[:n], voice=v, **kw)),
                         ("to_fine", lambda: sem._to_fine_in_groups(coarse.codes, 0.5, 1, None, history=None if v is None else v.codes) if n > 64
                          else sem.to_fine(coarse.codes, seed=1, history=None if v is None else v.codes))):
            fn()
            _, stage[what], _ = timed(fn, args.reps)
        lines.append(f"{name}: {ms:9.1f} ms (spread {spread:.1f} ms), {frames} generated frames = {frames / 75.0:.2f} s of audio, "
                     f"{frames / 75.0 / (ms / 1e3):.2f} audio s / wall s; of it to_acoustic {stage['to_acoustic']:.1f} ms ({len(coarse.ticks)} ticks, "
                     f"{sum(t[2] for t in coarse.ticks)} prefill tokens), to_fine {stage['to_fine']:.1f} ms")
        print(lines[-1])
    dec = sem._gpt()
    last = plan(N_SOURCE)[-1]   # that tool's sources (the first 16 drawn above) and its draws at --batches 16
    u = np.random.Generator(np.random.Philox(1)).random((16, r * last[0] + last[2] + 2 * MAX_NEW), dtype=np.float32)
    call = lambda: dec.to_acoustic_long(srcs[:16], window=S, hop=H, max_new_tokens=MAX_NEW, uniforms=u)   # noqa: E731
    call()
    _, ms, spread = timed(call, args.reps)
    lines.append(f"prompt-free to_acoustic_long, B=16 (the leg of tools/long_form_bench.py): this build {ms:.1f} ms (spread {spread:.1f} ms)")
    if args.parent_ms is not None:
        diff = ms - args.parent_ms
        recorded = args.recorded_spread_ms if args.recorded_spread_ms is not None else recorded_b16_spread_ms()
        verdict = "within" if diff <= recorded else "MORE THAN"
        lines.append(f"the same leg on the parent commit's build, same machine: {args.parent_ms:.1f} ms (spread {args.parent_spread_ms or 0.0:.1f} ms); this build - parent = "
                     f"{diff:+.1f} ms, {verdict} the {recorded:.1f} ms spread profiles/long_form.txt records for it")
    else:
        lines.append("the parent commit's build was not measured in this run")
    print("\n".join(lines[-2:]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
