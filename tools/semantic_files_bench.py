"""Measure the fine stage's window queue and ``AudioToken.to_audio_batch_files`` and write profiles/semantic_files.txt.

Models: the full-size synthetic ones of §19 / §20 and §18: a 12-layer GPT (block 1024) at the product geometry (S = 250, H = 124, r = 3),
``max_new_tokens`` 64, and a 12-layer / 768 fine model at W = 1024. Wall time around the calls with their closing copies, one warm-up, the median of
``--reps`` runs and their spread (max - min).

Fine stage alone, on the same random coarse codes for both legs, for two row sets: (1) the frames of §20's 256 sources of 100 to 1 500 ids (3 frames per
2 ids); (2) a skewed set, four rows of about 20 000 frames among 252 short ones. Baseline: ``to_fine`` in groups of 64 in source order
(``AudioToken._to_fine_in_groups``). Against it: ``to_fine(slots=64)``.

The file route end to end on set (1): 256 semantic token files on ``--shm`` through ``to_audio_batch_files``; audio seconds per wall second and the
shares of the GPT, the fine stage, the decode and the writes from ``run_timings``. Baseline: a hand-written loop of ``to_audio(..., slots=64)`` +
``save_audio`` over the same sources.

Both baselines use nothing this feature added, so ``--baseline-only`` runs on a checkout without it (the parent commit's build, since this change
touches the kernels the grouped call runs) and writes a JSON file that ``--baseline-file`` takes back.

    python tools/semantic_files_bench.py [--reps 3] [--baseline-only --baseline-file F | --baseline-file F] [--no-e2e]
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.audio_io import save_audio  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402

S, H, MAX_NEW = 250, 124, 64
BLOCK = 1024


def timed(fn, reps):
    out, ms = None, []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ms), max(ms) - min(ms)


def row_sets(n):
    rng = np.random.default_rng(20)
    ids = rng.integers(100, 1501, size=n)                         # §20's sources
    first = [int(3 * N // 2) for N in ids]
    skew = [int(x) for x in np.random.default_rng(23).integers(100, 901, size=n)]
    for at, T in zip((7, 70, 133, 196), (20000, 19500, 20500, 19990)):  # one long row in each group of 64
        skew[at % n] = T
    return ids, {"sources": first, "skewed": skew}


def coarse_rows(lens, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 1024, size=(2, T)) for T in lens]


def windows(T):
    return (-(-(T - BLOCK) // (BLOCK // 2)) if T > BLOCK else 0) + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--baseline-file", default=None, help="written by --baseline-only on the parent commit's build, read back otherwise")
    ap.add_argument("--no-e2e", action="store_true")
    ap.add_argument("--shm", default="/dev/shm/semantic_files_bench")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "semantic_files.txt"))
    args = ap.parse_args()
    cfg = Wav2VecBertDecoderConfig()
    gpt = W.synth_gpt_weights(n_layer=12, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    fine_w = W.synth_fine_weights(12, 768, BLOCK, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device="cuda:0", decoder_weights=gpt, fine_weights=fine_w)
    ids_lens, sets = row_sets(args.sources)
    rng = np.random.default_rng(21)
    srcs = [rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=int(N)).astype(np.int64) for N in ids_lens]
    base = {"sources": args.sources}
    lines = [f"tools/semantic_files_bench.py on {torch.cuda.get_device_name(0)}: {args.sources} rows; 12-layer synthetic GPT (block 1024, S={S} H={H} r=3, "
             f"max_new_tokens={MAX_NEW}), 12-layer / 768 synthetic fine model (W = {BLOCK}), temperature 0.5; wall time around the calls with their closing "
             f"copies, one warm-up, {args.reps} runs each (median, spread = max - min)"]

    # ---- the fine stage alone
    for name, lens in sets.items():
        rows = coarse_rows(lens, 31)
        n_win = sum(windows(T) for T in lens)
        lines.append(f"fine stage alone, set '{name}': {len(lens)} rows of {min(lens)} to {max(lens)} frames ({sum(lens)} frames, {n_win} windows)")
        if args.baseline_only:
            grouped = lambda: sem._to_fine_in_groups(rows, 0.5, 3, None)   # noqa: E731
            grouped()
            _, ms, spread = timed(grouped, args.reps)
            lockstep_passes = sum(max(windows(T) for T in lens[at:at + 64]) for at in range(0, len(lens), 64))
            base["fine_" + name] = dict(ms=ms, spread=spread, passes=lockstep_passes)
            print(f"grouped, {name}: {ms:.1f} ms (spread {spread:.1f}), {lockstep_passes} passes", flush=True)
            continue
        queue = lambda: sem.to_fine(rows, temperature=0.5, seed=3, slots=64)   # noqa: E731
        queue()
        out, ms, spread = timed(queue, args.reps)
        line = (f"  to_fine(slots=64): {ms:9.1f} ms (spread {spread:.1f} ms), {len(out.passes)} passes, {np.mean([p[0] for p in out.passes]):.1f} windows per pass, "
                f"{ms / n_win:.2f} ms per window, {sum(lens) / (ms / 1e3):,.0f} frames/s")
        lines.append(line)
        print(line, flush=True)

    # ---- the file route end to end
    if not args.no_e2e:
        shutil.rmtree(args.shm, ignore_errors=True)
        tree, out_dir = os.path.join(args.shm, "tokens"), os.path.join(args.shm, "audio")
        os.makedirs(tree)
        for i, s in enumerate(srcs):
            np.save(os.path.join(tree, f"s{i:04d}.npy"), s[None])
        kw = dict(window=S, hop=H, max_new_tokens=MAX_NEW, slots=64)
        if args.baseline_only:
            def loop():
                audio, _, _ = sem.to_audio(srcs, long_form=True, seed=5, **kw)
                os.makedirs(out_dir, exist_ok=True)
                for i, a in enumerate(audio):
                    save_audio(a, os.path.join(out_dir, f"s{i:04d}.wav"), 24000)
                return sum(a.shape[-1] for a in audio) / 24000.0
            loop()
            audio_s, ms, spread = timed(loop, args.reps)
            base["e2e"] = dict(ms=ms, spread=spread, audio_s=audio_s)
            print(f"hand loop: {ms:.1f} ms (spread {spread:.1f}), {audio_s:.1f} s of audio", flush=True)
        else:
            def route():
                sem.to_audio_batch_files(8, out_dir, token_dir=tree, seed=5, fine_slots=64, round_files=1024, **kw)
                return dict(sem.run_summary), dict(sem.run_timings)
            route()
            (summary, t), ms, spread = timed(route, args.reps)
            audio_s = summary["generated_frames"] / 75.0
            decode_s = t["total_s"] - t["gpt_s"] - t["fine_s"] - t["save_s"]
            line = (f"to_audio_batch_files, set 'sources' as files on {os.path.dirname(args.shm)}, batch_size 8, one clip per file, one round: {ms:9.1f} ms "
                    f"(spread {spread:.1f} ms), {audio_s:.1f} s of audio, {audio_s / (ms / 1e3):.2f} audio s / wall s; last run's host seconds: GPT "
                    f"{t['gpt_s']:.2f} ({100 * t['gpt_s'] / t['total_s']:.1f} %), fine {t['fine_s']:.2f} ({100 * t['fine_s'] / t['total_s']:.1f} %), writes "
                    f"{t['save_s']:.2f} ({100 * t['save_s'] / t['total_s']:.1f} %), decode and the rest {decode_s:.2f} ({100 * decode_s / t['total_s']:.1f} %); "
                    f"{summary['gpt_ticks']} GPT ticks, {summary['fine_passes']} fine passes, {summary['batches']} decode batches")
            lines.append(line)
            print(line, flush=True)
        shutil.rmtree(args.shm, ignore_errors=True)
    else:
        lines.append("the file route end to end: UNMEASURED in this run")

    if args.baseline_only:
        with open(args.baseline_file, "w") as f:
            json.dump(base, f)
        print("BASELINE " + json.dumps(base))
        return
    if args.baseline_file and os.path.exists(args.baseline_file):
        with open(args.baseline_file) as f:
            base = json.load(f)
        assert base["sources"] == args.sources, "the baseline was taken on another workload"
        for name in sets:
            b = base["fine_" + name]
            lines.append(f"baseline (the parent commit's build, same visit), set '{name}': to_fine in groups of 64 in source order: {b['ms']:9.1f} ms "
                         f"(spread {b['spread']:.1f} ms), {b['passes']} passes")
        if "e2e" in base:
            b = base["e2e"]
            lines.append(f"baseline (the parent commit's build, same visit): to_audio(long_form=True, slots=64) over all sources + save_audio per file: "
                         f"{b['ms']:9.1f} ms (spread {b['spread']:.1f} ms), {b['audio_s']:.1f} s of audio, {b['audio_s'] / (b['ms'] / 1e3):.2f} audio s / wall s")
    else:
        lines.append("the baselines (grouped to_fine; the hand-written to_audio loop) on the parent commit's build: UNMEASURED in this run")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
