#!/usr/bin/env python3
"""Stream pools: whole-file streaming of many long clips one at a time against the same clips through a pool (writes profiles/stream_pool.json and
profiles/stream_pool.txt).

    python tools/stream_pool_bench.py [--out-dir profiles] [--clips 64] [--seconds 300] [--push-seconds 10] [--reps 3] [--warmup 1]

Needs the MI355X (no CPU path: without a device it fails). Synthetic weights, seeded inputs generated on the device, so nothing is read from disk and no
host-to-device copy is inside a timed window. Every figure is device-event time around calls that end in the product path's own synchronisation (the status
read of every push), median of --reps runs with the min .. max spread; the two routes of a pair alternate. In one run it reports, for encode and for decode:

  one at a time   AcousticStream(batch=1) / AcousticDecodeStream(batch=1), one clip after the other: the path as it was before the pools (the baseline)
  pool            the same clips, all open at once in a pool of --clips slots
  lockstep        AcousticStream(batch=clips): what the pool could reach at best on equal-length clips (no gather / scatter, no grouping)

and the time of one gather + one scatter at B = clips against the time of one pooled push.
"""
import argparse
import json
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--clips", type=int, default=64)
ap.add_argument("--seconds", type=int, default=300)
ap.add_argument("--push-seconds", type=int, default=10)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--warmup", type=int, default=1)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import AcousticDecoderConfig, AcousticEncoderConfig  # noqa: E402
from audiotoken_amd.decoder import AcousticDecoder  # noqa: E402
from audiotoken_amd.encoder import AcousticEncoder  # noqa: E402

SR, HOP, RATE = 24000, 320, 75
LINES = []
RESULT = {"clips": args.clips, "seconds_per_clip": args.seconds, "push_seconds": args.push_seconds, "reps": args.reps, "warmup": args.warmup}


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


def alternate(routes, reps, warmup):
    """{name: [ms per run]}: every route warmed up, then the routes in turn, reps times."""
    for fn in routes.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in routes}
    for _ in range(reps):
        for name, fn in routes.items():
            ms[name].append(once(fn))
    return ms


def report(what, ms, audio_s):
    out = {}
    for name, v in ms.items():
        med = statistics.median(v)
        out[name] = {"ms_median": med, "ms_min": min(v), "ms_max": max(v), "audio_s_per_s": audio_s / (med / 1e3)}
        say(f"{what:7s} {name:14s} {med:10.1f} ms [{min(v):.1f} .. {max(v):.1f}]  = {audio_s / (med / 1e3):10.0f} audio-s/s")
    return out


def copies(pool, model, B, reps=200):
    """ms of one gather + one scatter at B rows, slots reversed (the copies are what the product calls: pool.gather_scatter is a transaction without its push)."""
    slots = list(range(B))[::-1]
    pool.gather_scatter(slots, fresh=True)      # a state the handle knows, for the scatter
    for _ in range(9):
        pool.gather_scatter(slots)
    torch.cuda.synchronize()
    return once(lambda: [pool.gather_scatter(slots) for _ in range(reps)]) / reps


def encode_side():
    B, N, n = args.clips, args.seconds * SR, args.push_seconds * SR
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    x = 0.1 * torch.randn((B, N), device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(1))

    def one_at_a_time():
        for b in range(B):
            st = enc.new_stream(1)
            for pos in range(0, N, n):
                st.push(x[b:b + 1, pos:pos + n])
            st.flush()

    def pooled():
        pool = enc.new_stream_pool(B)
        ids = [pool.open() for _ in range(B)]
        for pos in range(0, N, n):
            pool.push({sid: x[b, pos:pos + n] for b, sid in enumerate(ids)})
        pool.flush(ids)

    def lockstep():
        st = enc.new_stream(B)
        for pos in range(0, N, n):
            st.push(x[:, pos:pos + n])
        st.flush()

    # the three routes give the same tokens (checked on the first push + one more, outside the timed windows)
    st, pool = enc.new_stream(B), enc.new_stream_pool(B)
    ids = [pool.open() for _ in range(B)]
    same = True
    for pos in (0, n):
        ref = st.push(x[:, pos:pos + n])
        got = pool.push({sid: x[b, pos:pos + n] for b, sid in enumerate(ids)})
        same = same and all(torch.equal(got[sid], ref[b]) for b, sid in enumerate(ids))
    say(f"encode: pooled tokens torch.equal the lockstep stream's on two pushes: {same}")
    ms = alternate({"one at a time": one_at_a_time, "pool": pooled, "lockstep": lockstep}, args.reps, args.warmup)
    res = report("encode", ms, B * args.seconds)
    per_push = res["pool"]["ms_median"] / (N // n)
    gs = copies(pool, enc, B)
    say(f"encode  gather + scatter at B = {B}: {gs:.4f} ms per push of {per_push:.1f} ms = {100 * gs / per_push:.2f} % of a pooled push")
    res.update({"tokens_equal_lockstep": same, "gather_scatter_ms": gs, "pooled_push_ms": per_push, "pool_over_one_at_a_time":
                res["one at a time"]["ms_median"] / res["pool"]["ms_median"], "pool_over_lockstep": res["pool"]["ms_median"] / res["lockstep"]["ms_median"]})
    return res


def decode_side():
    B, T, t = args.clips, args.seconds * RATE, args.push_seconds * RATE
    dec = AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=True))
    toks = torch.randint(0, 1024, (B, 8, T), dtype=torch.long, device="cuda:0", generator=torch.Generator(device="cuda:0").manual_seed(2))

    def one_at_a_time():
        for b in range(B):
            st = dec.new_stream(1)
            for pos in range(0, T, t):
                st.push(toks[b:b + 1, :, pos:pos + t])
            st.flush()

    def pooled():
        pool = dec.new_stream_pool(B)
        ids = [pool.open() for _ in range(B)]
        for pos in range(0, T, t):
            pool.push({sid: toks[b, :, pos:pos + t] for b, sid in enumerate(ids)})
        pool.flush(ids)

    def lockstep():
        st = dec.new_stream(B)
        for pos in range(0, T, t):
            st.push(toks[:, :, pos:pos + t])
        st.flush()

    st, pool = dec.new_stream(B), dec.new_stream_pool(B)
    ids = [pool.open() for _ in range(B)]
    same = True
    for pos in (0, t):
        ref = st.push(toks[:, :, pos:pos + t])
        got = pool.push({sid: toks[b, :, pos:pos + t] for b, sid in enumerate(ids)})
        same = same and all(torch.equal(got[sid], ref[b]) for b, sid in enumerate(ids))
    say(f"decode: pooled audio torch.equal the lockstep stream's on two pushes: {same}")
    ms = alternate({"one at a time": one_at_a_time, "pool": pooled, "lockstep": lockstep}, args.reps, args.warmup)
    res = report("decode", ms, B * args.seconds)
    per_push = res["pool"]["ms_median"] / (T // t)
    gs = copies(pool, dec, B)
    say(f"decode  gather + scatter at B = {B}: {gs:.4f} ms per push of {per_push:.1f} ms = {100 * gs / per_push:.2f} % of a pooled push")
    res.update({"audio_equal_lockstep": same, "gather_scatter_ms": gs, "pooled_push_ms": per_push, "pool_over_one_at_a_time":
                res["one at a time"]["ms_median"] / res["pool"]["ms_median"], "pool_over_lockstep": res["pool"]["ms_median"] / res["lockstep"]["ms_median"]})
    return res


def main():
    if not torch.cuda.is_available():
        raise SystemExit("stream_pool_bench needs the GPU: there is nothing to measure on a CPU")
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    say(f"tools/stream_pool_bench.py on {torch.cuda.get_device_name(0)}: {args.clips} clips x {args.seconds} s, pushes of {args.push_seconds} s, K = 8, "
        f"synthetic weights seed 0, device-event ms, median of {args.reps} [min .. max], warm-up {args.warmup}, routes alternating")
    say()
    RESULT["device"] = torch.cuda.get_device_name(0)
    RESULT["encode"] = encode_side()
    torch.cuda.empty_cache()
    say()
    RESULT["decode"] = decode_side()
    say()
    for side in ("encode", "decode"):
        r = RESULT[side]
        say(f"{side}: pool / one at a time = {r['pool_over_one_at_a_time']:.1f} x the rate; pool time / lockstep time = {r['pool_over_lockstep']:.3f}; "
            f"gather + scatter = {100 * r['gather_scatter_ms'] / r['pooled_push_ms']:.2f} % of a push")
        # the two statements that must hold
        say(f"{side}: pooled rate not below one at a time: {r['pool_over_one_at_a_time'] >= 1.0}; gather + scatter below 5 % of a push: "
            f"{r['gather_scatter_ms'] < 0.05 * r['pooled_push_ms']}")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "stream_pool.json"), "w") as f:
        json.dump(RESULT, f, indent=1)
        f.write("\n")
    with open(os.path.join(out_dir, "stream_pool.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/stream_pool.json and stream_pool.txt")


if __name__ == "__main__":
    main()
