"""Measure the long form of semantic-to-acoustic generation and write profiles/long_form.txt.

Workload: sources of 1500 semantic ids (one 30 s chunk) through the full-size 12-layer synthetic GPT at the product geometry (S = 250, H = 124, r = 3: 12
windows a source), B = 1, 16, 64 sources a call. Recorded per B: the wall time of ``to_acoustic_long`` (median of ``--reps`` runs and their spread), audio
seconds per wall second (2 ids a frame, 75 frames a second), and the share of the prefills, measured as the same window prompts run through ``generate``
for one new token. The by-hand leg drives the same windows of ONE source through ``generate``, prompt rebuilt on the host each time; by hand, B sources
cost B times that, one after the other. It uses nothing this feature added, so ``--by-hand-only`` runs on a checkout without it (and prints instead of
writing the profile).

    python tools/long_form_bench.py [--batches 1,16,64] [--reps 3] [--by-hand-only] [--by-hand-ms X --by-hand-spread-ms Y]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.semantic_decoder import SemanticToAcoustic  # noqa: E402

S, H, r = 250, 124, 3
N_SOURCE = 1500
MAX_NEW = 64           # the final window's budget: at r ids a source id, the 10 source ids past window 10's end need 30


def plan(N):
    """(source_start, source_len, carry, new_ids or None) per window: the rule of DESIGN.md §19, restated so that this leg needs nothing but ``generate``."""
    n = 1 if N <= S else -(-(N - S) // H) + 1
    return [(k * H, min(S, N - k * H), r * (S - H) if k else 0, None if k == n - 1 else r * S - (r * (S - H) if k else 0)) for k in range(n)]


def rules(cfg, final):
    a, n = cfg.ACOUSTIC_OFFSET, cfg.codebook_size
    return [[a, a + n, cfg.STOP_TOKEN, cfg.STOP_TOKEN + 1] if final else [a, a + n, 0, 0], [a + n, a + 2 * n, 0, 0]]


def prompt_of(cfg, src, stream, win):
    start, n_src, carry, _ = win
    return np.concatenate([src[start:start + n_src] + cfg.SEMANTIC_OFFSET, [cfg.INFER_TOKEN], stream[r * start:r * start + carry]]).astype(np.int32)


def by_hand(dec, cfg, src, u_row):
    stream = np.zeros(0, dtype=np.int64)
    windows = plan(len(src))
    for k, win in enumerate(windows):
        final = k == len(windows) - 1
        base = r * win[0] + win[2]
        n_new = MAX_NEW if final else win[3]
        ids, _, _ = dec.generate([prompt_of(cfg, src, stream, win)], n_new, 0.8, 100, cfg.STOP_TOKEN if final else -1, uniforms=u_row[None, base:base + n_new],
                                 allow=rules(cfg, final))
        stream = np.concatenate([stream, ids[0].numpy()])
    return stream


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), max(ms) - min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--by-hand-only", action="store_true")
    ap.add_argument("--by-hand-ms", type=float, default=None, help="the by-hand leg as measured elsewhere (a checkout without the feature)")
    ap.add_argument("--by-hand-spread-ms", type=float, default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "long_form.txt"))
    args = ap.parse_args()
    cfg = Wav2VecBertDecoderConfig()
    w = W.synth_gpt_weights(n_layer=args.layers, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    dec = SemanticToAcoustic(cfg, device="cuda:0", weights=w)
    rng = np.random.default_rng(0)
    batches = [int(b) for b in args.batches.split(",")]
    srcs = [rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=N_SOURCE).astype(np.int64) for _ in range(max(batches))]
    last = plan(N_SOURCE)[-1]
    cap = r * last[0] + last[2] + MAX_NEW
    u = np.random.Generator(np.random.Philox(1)).random((max(batches), cap + MAX_NEW), dtype=np.float32)
    lines = [f"long form: {N_SOURCE}-id sources, {args.layers}-layer synthetic GPT (vocab {cfg.VOCAB_SIZE}, block 1024), S={S} H={H} r={r}, "
             f"{len(plan(N_SOURCE))} windows a source, max_new_tokens={MAX_NEW}, {args.reps} runs each (median, spread = max - min)"]

    by_hand(dec, cfg, srcs[0], u[0])   # warm-up
    hand_stream, hand_ms, hand_spread = timed(lambda: by_hand(dec, cfg, srcs[0], u[0]), args.reps)
    where = "this build"
    print(f"by hand, one source: {hand_ms:.1f} ms (spread {hand_spread:.1f} ms), {len(hand_stream)} ids")
    if args.by_hand_only:
        return
    if args.by_hand_ms is not None:
        lines.append(f"by hand on this build, one source: {hand_ms:.1f} ms (spread {hand_spread:.1f} ms)")
        hand_ms, hand_spread, where = args.by_hand_ms, args.by_hand_spread_ms or 0.0, "the parent commit's build"
    lines.append(f"by hand ({where}), one source through {len(plan(N_SOURCE))} generate calls: {hand_ms:.1f} ms (spread {hand_spread:.1f} ms), "
                 f"{len(hand_stream)} ids = {len(hand_stream) / 150.0:.2f} s of audio, {len(hand_stream) / 150.0 / (hand_ms / 1e3):.2f} audio s / wall s")

    for B in batches:
        rows = srcs[:B]
        call = lambda: dec.to_acoustic_long(rows, window=S, hop=H, max_new_tokens=MAX_NEW, uniforms=u[:B])   # noqa: E731
        call()   # warm-up
        out, ms, spread = timed(call, args.reps)
        if B == 1:
            assert np.array_equal(out.ids[0].numpy() + cfg.ACOUSTIC_OFFSET, hand_stream), "the device-driven row is the by-hand chain, id for id"
        audio_s = sum(len(i) for i in out.ids) / 150.0
        # the prefills alone: every pass's prompts, rebuilt from the result, through generate for one token
        streams = [i.numpy() + cfg.ACOUSTIC_OFFSET for i in out.ids]
        passes = [[prompt_of(cfg, rows[b], streams[b], win) for b, win in ((b, plan(N_SOURCE)[k]) for b in range(B))] for k in range(len(plan(N_SOURCE)))]

        def prefills():
            for prompts in passes:
                dec.generate(prompts, 1, 0.8, 100, -1, uniforms=np.full((B, 1), 0.5, dtype=np.float32))

        prefills()
        _, pre_ms, _ = timed(prefills, args.reps)
        lines.append(f"B={B:2d}: device-driven {ms:9.1f} ms (spread {spread:.1f} ms), {audio_s:7.2f} s of audio, {audio_s / (ms / 1e3):7.2f} audio s / wall s; "
                     f"prefills (with one step each) {pre_ms:.1f} ms = {100.0 * pre_ms / ms:.1f} % of the call; "
                     f"by hand, one source at a time: {B * hand_ms:.1f} ms, ratio {B * hand_ms / ms:.2f}x")
        print(lines[-1])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
