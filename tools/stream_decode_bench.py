#!/usr/bin/env python3
"""Streaming acoustic decode: equality with one-shot and what a push costs (writes profiles/stream_decode.txt).

    python tools/stream_decode_bench.py [--out profiles/stream_decode.txt] [--quick] [--parent-tree DIR]

Needs the MI355X (no CPU path: without a device it fails). Synthetic weights and seeded random tokens, so nothing is read from disk.
Per-push latencies are WALL times of ``push`` (it returns after the status word was read, i.e. when the audio is complete): median of --reps
pushes after warm-up, with the spread. Whole-clip times are device events around the calls.
``--parent-tree DIR`` names a built checkout of the parent commit: its one-shot decode of 64 x 10 s is then timed in child processes that
alternate with this commit's (``--oneshot-only`` is that child's mode), because the one-shot path must not have become slower.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
ap.add_argument("--quick", action="store_true", help="skip the 600 s comparison")
ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (one-shot decode is timed there too)")
ap.add_argument("--oneshot-only", action="store_true", help="print one JSON line with the one-shot decode time at 64 x 10 s and exit")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package is measured")
args = ap.parse_args()
ROOT = os.path.abspath(args.root)
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import AcousticDecoderConfig  # noqa: E402
from audiotoken_amd.decoder import AcousticDecoder  # noqa: E402

HOP = 320
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def tokens(B, T, seed, K=8):
    return torch.randint(0, 1024, (B, K, T), dtype=torch.long, generator=torch.Generator().manual_seed(seed)).cuda()


def timed(fn, reps, warmup):
    """Median / min / max milliseconds of fn() by device events (fn ends in whatever synchronisation the product path has)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def one_shot_64x10(dec, reps, warmup):
    toks = tokens(64, 750, 5)

    def one_shot():
        dec(toks)
        dec.last_status()
    return timed(one_shot, reps, warmup)


def stream_all(dec, toks, sizes):
    st = dec.new_stream(toks.shape[0])
    parts, pos = [], 0
    for n in sizes:
        parts.append(st.push(toks[:, :, pos:pos + n]).clone())
        pos += n
    return torch.cat(parts, dim=1), parts


def equality(dec):
    say("== 1. streaming vs one-shot decode, same handle, same tokens, default options ==")
    say("(a stream's first push selects one-shot decode's kernels: torch.equal holds for it at every shape below; later pushes run the same arithmetic on")
    say(" other tiles and are compared by value)")
    rows = [(1, 150, [150]), (1, 150, [7] + [1] * 143), (3, 150, [75, 75]), (64, 40, [7] + [1] * 33), (64, 750, [75] * 10), (1, 22500, [750] * 30)]
    for B, T, sizes in rows:
        toks = tokens(B, T, 100 + B)
        one = dec(toks).reshape(B, -1).clone()
        first = dec(toks[:, :, :sizes[0]].contiguous()).reshape(B, -1).clone()
        wav, parts = stream_all(dec, toks, sizes)
        d = (wav - one).abs().max().item()
        say(f"B {B:3d}  T {T:6d}  pushes of {sizes[0]}{' then ' + str(sizes[1]) if len(sizes) > 1 else ''}: first push torch.equal one-shot of its frames "
            f"{torch.equal(parts[0], first)}; whole stream torch.equal one-shot {torch.equal(wav, one)}, max |diff| {d:.3e} at scale {one.abs().max().item():.2f}")
    say()


def push_latency(dec, reps):
    say("== 2. per-push latency, B = 1, mid-stream (WALL ms per push incl. the status read: median [min .. p90 .. max]) ==")
    for t in (1, 2, 5, 15, 75):
        toks = tokens(1, 75 + t, 50 + t)
        st = dec.new_stream(1)
        st.push(toks[:, :, :75])
        piece = toks[:, :, 75:].contiguous()
        for _ in range(20):
            st.push(piece)
        torch.cuda.synchronize()
        w = []
        for _ in range(reps):
            t0 = time.perf_counter()
            st.push(piece)
            w.append((time.perf_counter() - t0) * 1e3)
        w.sort()
        med = statistics.median(w)
        say(f"t {t:2d} frames ({t / 75 * 1000:6.1f} ms of audio): {med:7.3f} [{w[0]:7.3f} .. {w[int(0.9 * (len(w) - 1))]:7.3f} .. {w[-1]:7.3f}] ms  = {med / (t / 75 * 1000):.4f} x real time")
    say()


def versus(dec, B, T, step, reps, warmup, what):
    toks = tokens(B, T, 7 + B)
    say(f"-- {what}: B = {B}, {T} frames ({T / 75:.0f} s) per clip, pushes of {step} frames --")

    def one_shot():
        dec(toks)
        dec.last_status()

    def streamed():
        st = dec.new_stream(B)
        for t0 in range(0, T, step):
            st.push(toks[:, :, t0:t0 + step])
        st.flush()

    lib, h = dec._h.lib, dec._h.handle
    m2, lo2, hi2 = timed(streamed, reps, warmup)
    try:
        m1, lo1, hi1 = timed(one_shot, reps, warmup)
        m2b, _, _ = timed(streamed, reps, 0)          # again, after the other: the two alternate
        say(f"one-shot {m1:9.3f} [{lo1:.3f} .. {hi1:.3f}] ms;  streamed {m2:9.3f} [{lo2:.3f} .. {hi2:.3f}] ms (repeat after the one-shot runs: {m2b:.3f});  ratio {m2 / m1:.3f}")
    except Exception as e:   # an argument error or an allocation failure of the one-shot call at this length: the streamed figure stands alone
        say(f"one-shot decode failed at this length ({type(e).__name__}: {str(e)[:160]});  streamed {m2:9.3f} [{lo2:.3f} .. {hi2:.3f}] ms")
    say(f"workspace: one-shot {lib.at_encodec_decode_workspace_bytes(h, B, T) / 2**20:.1f} MiB, one push {lib.at_encodec_decode_stream_workspace_bytes(h, B, step) / 2**20:.1f} MiB "
        f"+ state {2 * lib.at_encodec_decode_stream_state_bytes(h, B) / 2**10:.1f} KiB")
    say()


def child(root, reps, warmup):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "--oneshot-only", "--root", root, "--reps", str(reps), "--warmup", str(warmup)],
                         cwd=root, capture_output=True, text=True, timeout=600)
    if out.returncode != 0:
        raise SystemExit(f"child in {root} failed ({out.returncode}):\n{out.stdout}\n{out.stderr}")
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stream_decode_bench needs the GPU: there is nothing to measure on a CPU")
    dec = AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=True))
    if args.oneshot_only:
        med, lo, hi = one_shot_64x10(dec, args.reps, args.warmup)
        print(json.dumps({"root": ROOT, "one_shot_64x10s_ms": med, "min": lo, "max": hi}))
        return
    out = args.out or os.path.join(ROOT, "profiles", "stream_decode.txt")
    say(f"tools/stream_decode_bench.py on {torch.cuda.get_device_name(0)}; K = 8, synthetic weights seed 0, reps {args.reps}, warm-up {args.warmup}")
    say()
    equality(dec)
    push_latency(dec, max(args.reps, 200))
    say("== 3. streamed against one-shot, same build, same box ==")
    versus(dec, 64, 750, 75, args.reps, args.warmup, "64 clips x 10 s in 1 s pushes")
    if not args.quick:
        versus(dec, 1, 45000, 750, max(3, args.reps // 2), 1, "one 600 s clip in 10 s pushes")
    say("== 4. one-shot decode at 64 x 10 s, this commit against the parent commit (child processes, alternating) ==")
    del dec
    torch.cuda.empty_cache()
    if args.parent_tree:
        parent = os.path.abspath(args.parent_tree)
        rows = [child(r, args.reps, args.warmup) for r in (ROOT, parent, ROOT, parent)]
        for name, r in zip(("this commit", "parent", "this commit", "parent"), rows):
            say(f"{name:12s} {r['one_shot_64x10s_ms']:9.3f} [{r['min']:.3f} .. {r['max']:.3f}] ms")
        a = statistics.mean([rows[0]["one_shot_64x10s_ms"], rows[2]["one_shot_64x10s_ms"]])
        b = statistics.mean([rows[1]["one_shot_64x10s_ms"], rows[3]["one_shot_64x10s_ms"]])
        say(f"this commit / parent = {a / b:.4f}")
    else:
        say("unmeasured: no --parent-tree given")
    say()
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out}")


if __name__ == "__main__":
    main()
