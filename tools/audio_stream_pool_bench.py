"""Measure the semantic-to-audio stream pool and write profiles/audio_stream_pool.txt; nothing is asserted. One MI355X, the full-size 12-layer
synthetic GPT, the 12-layer / 768 synthetic fine model at W = 1024, the product geometry (S = 250, H = 124). ``n`` streams (default 1, 4, 16 and 64), each
pushed 25 ids per call until 1500 ids, then flushed: once through ``audio_stream_pool(streams=n, slots=min(n, 64), fine_slots=min(n, 16))``, and once, in the
same session, as ``n`` ``audio_stream()`` objects pushed the same pieces in the same order (the baseline: what the library could do before the pool). Per
leg: the wall time, the aggregate audio seconds per wall second, the wall time to the first non-empty audio piece, the device time of the GPT stage and of
the fine stage (HIP events around their library calls; the rest of the wall time is the decode, the copies and the host), and the state bytes. One run per
leg after one small warm-up; a stream count that is not run is written down as UNMEASURED.

    python tools/audio_stream_pool_bench.py [--streams 1 4 16 64] [--ids 1500] [--push 25]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402

S, H, MAX_NEW = 250, 124, 64
ALL = (1, 4, 16, 64)


def time_stage(model, store):
    """Wrap the model's library lookups: every stream / pool push is bracketed by two events on the current stream."""
    lookup = model._fn

    def fn(name):
        f = lookup(name)
        if name not in ("stream_push", "pool_push"):
            return f

        def call(*a):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            rc = f(*a)
            e1.record()
            store.append((e0, e1))
            return rc
        return call
    model._fn = fn


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, nargs="+", default=list(ALL))
    ap.add_argument("--ids", type=int, default=1500)
    ap.add_argument("--push", type=int, default=25)
    ap.add_argument("--layers", type=int, default=12)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "audio_stream_pool.txt"))
    args = ap.parse_args()
    cfg = Wav2VecBertDecoderConfig()
    gpt_w = W.synth_gpt_weights(n_layer=args.layers, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    fine_w = W.synth_fine_weights(args.layers, 768, 1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device="cuda:0", decoder_weights=gpt_w, fine_weights=fine_w)
    kw = dict(window=S, hop=H, max_new_tokens=MAX_NEW)
    gpt_ev, fine_ev = [], []
    warm = sem.audio_stream(seed=0, **kw)          # builds the three models, warms the kernels
    warm.push(np.arange(300) % 1000)
    warm.flush()
    time_stage(sem._gpt(), gpt_ev)
    time_stage(sem._fine(), fine_ev)
    rng = np.random.default_rng(0)
    lines = [f"semantic-to-audio stream pool: {args.layers}-layer synthetic GPT (vocab {cfg.VOCAB_SIZE}, block 1024), {args.layers}-layer / 768 synthetic fine model at "
             f"W = 1024, S={S} H={H}, max_new_tokens={MAX_NEW}; every stream pushed {args.push} ids per call until {args.ids} ids, then flushed; one run per leg after a "
             f"warm-up (no spread); GPT / fine: device time between HIP events around the stages' library calls; the baseline is that many audio_stream() objects, "
             f"pushed the same pieces, in the same session"]

    def stages():
        torch.cuda.synchronize()
        g = sum(a.elapsed_time(b) for a, b in gpt_ev)
        f = sum(a.elapsed_time(b) for a, b in fine_ev)
        gpt_ev.clear()
        fine_ev.clear()
        return g, f

    def report(name, wall, first, frames, g, f, extra):
        audio_s = frames / 75.0
        return (f"  {name}: wall {wall:.1f} ms, {audio_s:.1f} s of audio = {audio_s / (wall / 1e3):.2f} audio s / wall s; first audio after {first:.1f} ms; GPT stage "
                f"{g:.1f} ms ({100 * g / wall:.1f} %), fine stage {f:.1f} ms ({100 * f / wall:.1f} %), the rest {wall - g - f:.1f} ms ({100 * (wall - g - f) / wall:.1f} %){extra}")

    for n in ALL:
        if n not in args.streams:
            lines.append(f"{n} streams: UNMEASURED")
            continue
        srcs = [rng.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=args.ids).astype(np.int64) for _ in range(n)]
        cuts = list(range(0, args.ids, args.push))
        # ---- the pool
        pool = sem.audio_stream_pool(streams=n, slots=min(n, 64), fine_slots=min(n, 16), **kw)
        sids = [pool.open(seed=i) for i in range(n)]
        stages()
        t0, first, frames = time.perf_counter(), None, 0
        for at in cuts:
            out = pool.push({sid: src[at:at + args.push] for sid, src in zip(sids, srcs)})
            got = sum(a.shape[-1] for a in out.values()) // 320
            frames += got
            if first is None and got:
                first = (time.perf_counter() - t0) * 1e3
        out = pool.flush(sids)
        frames += sum(a.shape[-1] for a in out.values()) // 320
        torch.cuda.synchronize()
        wall_p = (time.perf_counter() - t0) * 1e3
        gp, fp = stages()
        dec_bytes = sum(s.numel() for s in [pool._decode._pool, *pool._decode._staging])
        lines.append(f"{n} streams:")
        lines.append(report("pool    ", wall_p, wall_p if first is None else first, frames, gp, fp,
                            f"; states: GPT {pool.state_bytes[0] / 2 ** 20:.1f} MiB, fine {pool.state_bytes[1] / 2 ** 20:.1f} MiB, decode pool {dec_bytes / 2 ** 20:.1f} MiB"))
        del pool
        # ---- the baseline: n solo streams
        solo = [sem.audio_stream(seed=i, **kw) for i in range(n)]
        stages()
        t0, first, frames = time.perf_counter(), None, 0
        for at in cuts:
            for st, src in zip(solo, srcs):
                piece = st.push(src[at:at + args.push])
                frames += piece.shape[-1] // 320
                if first is None and piece.shape[-1]:
                    first = (time.perf_counter() - t0) * 1e3
        for st in solo:
            frames += st.flush().shape[-1] // 320
        torch.cuda.synchronize()
        wall_s = (time.perf_counter() - t0) * 1e3
        gs, fs = stages()
        sb = solo[0].state_bytes
        lines.append(report("baseline", wall_s, wall_s if first is None else first, frames, gs, fs,
                            f"; states: {n} x (GPT {sb[0] / 2 ** 20:.1f} MiB, fine {sb[1] / 2 ** 20:.1f} MiB)"))
        lines.append(f"  pool / baseline: GPT stage time {gp / gs:.3f} ({gs / gp:.2f} x less), wall {wall_p / wall_s:.3f} ({wall_s / wall_p:.2f} x less)")
        del solo
        torch.cuda.empty_cache()
        print("\n".join(lines[-4:]), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
