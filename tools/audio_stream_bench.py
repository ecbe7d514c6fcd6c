"""Measure the semantic-to-audio stream and write profiles/audio_stream.txt; nothing is asserted. One MI355X, the full-size 12-layer
synthetic GPT, the 12-layer / 768 synthetic fine model at W = 1024, the product geometry (S = 250, H = 124). Sources of 250, 700 and 1500 ids, pushed 50
ids at a time (one second of speech each) and flushed. Per source, by the protocol of the other tools (one warm-up, the median of ``--reps`` runs and their
spread = max - min): the wall time to the first non-empty audio piece, the total wall time until ``flush()`` returns, and the bytes of the three states.
Beside them ``to_audio(tokens, long_form=True)`` of the same source: measured here with ``--offline`` on whatever build runs the tool (run it with that
flag on the parent commit's build, where the stream does not exist, and pass the figures back with ``--parent N:ms:spread:MiB`` per source).

    python tools/audio_stream_bench.py [--reps 3] [--sources 250 700 1500] [--offline] [--parent 250:ms:spread:MiB ...]
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

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402

S, H, MAX_NEW, PUSH = 250, 124, 64, 50


def med(xs):
    return statistics.median(xs), max(xs) - min(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sources", type=int, nargs="+", default=[250, 700, 1500])
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--offline", action="store_true", help="time to_audio(long_form=True) only: what the parent commit's build can run")
    ap.add_argument("--parent", nargs="*", default=[], help="N:ms:spread:MiB of to_audio(long_form=True) on the parent commit's build")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream.txt"))
    args = ap.parse_args()
    cfg = Wav2VecBertDecoderConfig()
    gpt = W.synth_gpt_weights(n_layer=args.layers, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    fine = W.synth_fine_weights(args.layers, 768, 1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device="cuda:0", decoder_weights=gpt, fine_weights=fine)
    parent = {int(p.split(":")[0]): [float(x) for x in p.split(":")[1:]] for p in args.parent}
    rng = np.random.default_rng(0)
    lines = [f"semantic-to-audio stream: {args.layers}-layer synthetic GPT (vocab {cfg.VOCAB_SIZE}, block 1024), {args.layers}-layer / 768 synthetic fine model at "
             f"W = 1024, S={S} H={H}, max_new_tokens={MAX_NEW}, pushes of {PUSH} ids; one warm-up, {args.reps} runs each (median, spread = max - min)"]
    kw = dict(window=S, hop=H, max_new_tokens=MAX_NEW, seed=1)
    for N in args.sources:
        src = rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=N).astype(np.int64)

        def offline():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            audio, _, _ = sem.to_audio(src, long_form=True, **kw)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, audio[0].shape[-1] // 320

        offline()
        torch.cuda.reset_peak_memory_stats()
        runs = [offline() for _ in range(args.reps)]
        off_ms, off_spread = med([x[0] for x in runs])
        off_mib = torch.cuda.max_memory_allocated() / 2 ** 20
        line = f"N={N}: to_audio(long_form=True) on this build {off_ms:.1f} ms (spread {off_spread:.1f} ms), {runs[0][1]} frames, peak allocated {off_mib:.1f} MiB"
        if N in parent:
            line += f"; on the parent commit's build {parent[N][0]:.1f} ms (spread {parent[N][1]:.1f} ms), peak allocated {parent[N][2]:.1f} MiB"
        else:
            line += "; the parent commit's build was not measured in this run"
        if not args.offline:
            st = sem.audio_stream(**kw)

            def streamed():
                st.reset()
                torch.cuda.synchronize()
                t0, first, frames = time.perf_counter(), None, 0
                for at in range(0, N, PUSH):
                    piece = st.push(src[at:at + PUSH])
                    frames += piece.shape[-1] // 320
                    if first is None and piece.shape[-1]:
                        first = (time.perf_counter() - t0) * 1e3
                piece = st.flush()
                frames += piece.shape[-1] // 320
                total = (time.perf_counter() - t0) * 1e3
                return (total if first is None else first), total, frames, first is None

            streamed()
            runs_s = [streamed() for _ in range(args.reps)]
            first_ms, first_spread = med([x[0] for x in runs_s])
            total_ms, total_spread = med([x[1] for x in runs_s])
            dec_bytes = sum(s.numel() for s in st._decode._state)
            states = sum(st.state_bytes) + dec_bytes
            line += (f"\n      stream: first audio after {first_ms:.1f} ms (spread {first_spread:.1f} ms{', at flush()' if runs_s[0][3] else ''}), total "
                     f"{total_ms:.1f} ms (spread {total_spread:.1f} ms), {runs_s[0][2]} frames; states {states / 2 ** 20:.1f} MiB (GPT {st.state_bytes[0] / 2 ** 20:.1f}, "
                     f"fine {st.state_bytes[1] / 2 ** 20:.1f}, decode {dec_bytes / 2 ** 20:.1f})")
        lines.append(line)
        print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
