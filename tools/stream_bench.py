#!/usr/bin/env python3
"""Streaming acoustic encode: equality with one-shot and what a push costs (writes profiles/stream_encode.txt).

    python tools/stream_bench.py [--out profiles/stream_encode.txt] [--quick]

Needs the MI355X (no CPU path: without a device it fails). Synthetic weights and seeded synthetic audio, so nothing is read from disk.
Times are HIP events on the launch stream around whole calls (median of --reps after --warmup calls of the same shape; the spread is printed);
the per-kernel-group figures are the library's own profile taps (at_encodec_profile), taken in a separate pass.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import AcousticEncoderConfig  # noqa: E402
from audiotoken_amd.encoder import AcousticEncoder  # noqa: E402

HOP = 320
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def wave(B, n, seed):
    return torch.from_numpy(W.synth_waveform(B, n, 24000, seed=seed)).cuda()


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


def stream_all(enc, x, sizes, keep_emb=True):
    st = enc.new_stream(x.shape[0])
    st.keep_embeddings = keep_emb
    cs, es, pos = [], [], 0
    for n in sizes:
        c = st.push(x[:, pos:pos + n])
        pos += n
        if c.shape[-1]:
            cs.append(c.clone())
            if keep_emb:
                es.append(st.last_embeddings.clone())
    c = st.flush()
    if c.shape[-1]:
        cs.append(c.clone())
        if keep_emb:
            es.append(st.last_embeddings.clone())
    return torch.cat(cs, -1), (torch.cat(es, 1) if keep_emb else None)


# ---- 1. equality ---------------------------------------------------------------------------------------------------------------------------
def equality(enc):
    say("== 1. streaming vs one-shot embeddings, same handle, same audio (default options unless stated) ==")
    base = 45 * HOP
    rows = [(1, base, [base]), (3, base, [6400, 6400, 1600]), (17, base, [2240] + [HOP] * 38), (81, base, [6400, 6400, 1600]),
            (1, 7500 * HOP, [240000] * 10)]
    for B, total, sizes in rows:
        x = wave(B, total, 1000 + B)
        c1, e1 = enc(x, None, return_embeddings=True)
        c1, e1 = c1.clone(), e1.clone()
        cs, es = stream_all(enc, x, sizes)
        say(f"B {B:3d}  total {total:8d} (= {total // HOP} frames)  pushes of {sizes[0]}{' then ' + str(sizes[1]) if len(sizes) > 1 else ''}: "
            f"embeddings torch.equal {torch.equal(es, e1)}, max |diff| {(es - e1).abs().max().item():.3e}, ids differing {int((cs != c1).sum())}")
    say()
    say("twins: totals for which the ONE-SHOT call selects other kernels than the frame-aligned mid-stream windows do; which option makes the windows take")
    say("the one-shot call's kernels again (the acoustic path has no per-stage taps besides emb_out, so the first differing kernel is found by switching")
    say("the fused / windowed-GEMM kernels off from the front of the stack until the embeddings are equal again):")
    ladders = [("defaults", {}),
               ("fused_stage0=0", {"fused_stage0": 0}),
               ("+ fused_stage1=0 fused_down64=0", {"fused_stage1": 0, "fused_down64": 0}),
               ("+ down128_x3=0", {"down128_x3": 0}),
               ("+ down256_x3=0", {"down256_x3": 0})]
    for tail, why in ((9, "odd N: the fused stage 0 needs N % 2 == 0"), (2, "N even, stage-1 length 7201: the fused stage 1 needs L % 4 == 0")):
        total = base + tail
        x = wave(3, total, 1003)
        say(f"  total {total} ({why})")
        done = {}
        for name, opts in ladders:
            for k, v in opts.items():
                enc.set_option(k, v)
                done[k] = 1
            c1, e1 = enc(x, None, return_embeddings=True)
            c1, e1 = c1.clone(), e1.clone()
            cs, es = stream_all(enc, x, [6400, 6400, total - 12800])
            d = (es - e1).abs()
            nfr = int((d.amax(dim=(0, 2)) > 0).sum())
            say(f"    {name:34s} equal {str(torch.equal(es, e1)):5s} max |diff| {d.max().item():.3e}  frames differing {nfr:2d} of {d.shape[1]}  ids differing {int((cs != c1).sum())}")
        for k in done:
            enc.set_option(k, 1)
    say()


# ---- 2. per-push latency -----------------------------------------------------------------------------------------------------------------
def push_latency(enc, reps, warmup):
    say("== 2. per-push latency, mid-stream (ms per push: median [min .. max]; the push includes the read of the status word) ==")
    for B in (1, 16, 64):
        for frames in (20, 75):
            n = frames * HOP
            x = wave(B, 75 * HOP + n, 50 + B)
            st = enc.new_stream(B)
            st.push(x[:, :75 * HOP])        # the stream's first push; every timed push is a mid-stream one of the same n samples
            piece = x[:, 75 * HOP:].contiguous()

            def one():
                st.push(piece)
            med, lo, hi = timed(one, reps, warmup)
            say(f"B {B:3d}  hop {frames:2d} frames ({frames / 75 * 1000:6.1f} ms of audio): {med:7.3f} [{lo:7.3f} .. {hi:7.3f}] ms  = {med / (frames / 75 * 1000):.4f} x real time per stream batch")
    say()


def groups(enc, fn):
    enc.enable_profile(True)
    fn()
    torch.cuda.synchronize()
    g = enc.read_profile()
    enc.enable_profile(False)
    return g


def merge(g):
    """Profile groups -> the note's kernel groups."""
    out = {}
    for k, (ms, n) in g.items():
        key = ("conv stack" if k.startswith(("stage0", "conv0", "res", "down")) else "lstm input projection" if k == "lstm_ih" else
               "lstm recurrence" if k == "lstm_rec" else "final conv" if k == "final_conv" else "rvq" if k == "rvq" else
               "state gather / scatter" if k == "stream_state" else k)
        a = out.setdefault(key, [0.0, 0])
        a[0] += ms
        a[1] += n
    return out


def versus(enc, B, seconds, reps, warmup, what):
    n_push = 240000
    pushes = seconds // 10
    total = n_push * pushes
    x = wave(B, total, 7 + B)
    say(f"-- {what}: B = {B}, {seconds} s per clip, {pushes} push(es) of 10 s --")

    def one_shot():
        c = enc(x, None)
        enc.last_status()
        return c

    def streamed():
        st = enc.new_stream(B)
        for i in range(pushes):
            st.push(x[:, i * n_push:(i + 1) * n_push])
        st.flush()

    m1, lo1, hi1 = timed(one_shot, reps, warmup)
    m2, lo2, hi2 = timed(streamed, reps, warmup)
    m1b, _, _ = timed(one_shot, reps, 0)          # again, after the other: the two alternate
    lib, h = enc._h.lib, enc._h.handle
    say(f"one-shot {m1:9.3f} [{lo1:.3f} .. {hi1:.3f}] ms (repeat after the streamed runs: {m1b:.3f});  streamed {m2:9.3f} [{lo2:.3f} .. {hi2:.3f}] ms;  ratio {m2 / m1:.3f}")
    say(f"workspace: one-shot {lib.at_encodec_workspace_bytes(h, B, total) / 2**20:.1f} MiB, one push {lib.at_encodec_stream_workspace_bytes(h, B, n_push) / 2**20:.1f} MiB "
        f"+ state {2 * lib.at_encodec_stream_state_bytes(h, B) / 2**10:.1f} KiB")
    g1, g2 = merge(groups(enc, one_shot)), merge(groups(enc, streamed))
    say(f"{'kernel group':26s} {'one-shot ms':>12s} {'launches':>9s} {'streamed ms':>12s} {'launches':>9s} {'diff ms':>9s}")
    t1 = t2 = 0.0
    for k in sorted(set(g1) | set(g2)):
        a, b = g1.get(k, [0.0, 0]), g2.get(k, [0.0, 0])
        t1 += a[0]
        t2 += b[0]
        say(f"{k:26s} {a[0]:12.3f} {a[1]:9d} {b[0]:12.3f} {b[1]:9d} {b[0] - a[0]:9.3f}")
    say(f"{'sum of groups':26s} {t1:12.3f} {'':9s} {t2:12.3f} {'':9s} {t2 - t1:9.3f}   (call time minus this = launch gaps, memsets, the status read, host)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_encode.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--quick", action="store_true", help="skip the 600 s comparison")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("stream_bench needs the GPU: there is nothing to measure on a CPU")
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    say(f"tools/stream_bench.py on {torch.cuda.get_device_name(0)}; n_q = 8, synthetic weights seed 0, reps {args.reps}, warm-up {args.warmup}")
    say()
    equality(enc)
    push_latency(enc, max(args.reps, 20), 5)
    say("== 3. streamed in 10 s pushes against one-shot, same build, same box ==")
    versus(enc, 64, 10, args.reps, args.warmup, "one push per clip (the flagship batch shape, quarter size)")
    versus(enc, 64, 30, args.reps, args.warmup, "three pushes per clip")
    if not args.quick:
        versus(enc, 1, 600, max(3, args.reps // 2), 1, "one long file")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
