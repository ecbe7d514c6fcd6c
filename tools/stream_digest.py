#!/usr/bin/env python3
"""What a fixed, seeded script of stream calls hands the library and gives back (audiotoken_amd/streaming.py: the two lockstep streams and the two
pools): the check of a change to the streams' host code that must not change what they do. Only the public API is used — constructors, ``open`` /
``push`` / ``flush`` / ``close`` / ``reset`` and the public attributes — so the same file runs against another checkout. Run it on two and diff:

    python tools/stream_digest.py --stub > a.txt                       # recording stubs and HostResampler, no device
    python tools/stream_digest.py --stub --root ../other > b.txt       # the package of another checkout
    python tools/stream_digest.py > c.txt                              # the real models with synthetic weights (AUDIOTOKEN_HIP_LIB selects the library)
    python tools/stream_digest.py --stub --time                        # also host seconds of the whole stub script: median of --reps runs [min .. max]

``--stub`` prints one line per stub call in order (hook, shape and sha256 of the tensor, ``final`` / ``started``, the slot list) and one per public
output (sha256, ``frames_emitted``, ``library_pushes``, ``live``, the resampler's ``launches``). The script: pushes of 0 samples, below one frame,
below 7 frames and then across them, exact multiples and ragged lengths; ``flush`` with nothing held, with a held tail and before the stream
started; ``reset`` and reuse; pools of 4 slots with opens, closes and flushes in mid-run, so that slots are reused and groups of different phase and
length meet in one call; 16 kHz int16 and 48 kHz float32 streams beside a model-rate one in one pool call; decode with K = 2 and K = 8 in one pool call.

The default mode (a few seconds on the device): bandwidth 6, a lockstep encode stream of B = 3 on 2240 + 3200 + 1000 samples with ``keep_embeddings``,
the same signal at 16 kHz, an encode pool of 4 slots on a ragged schedule, a lockstep decode stream of B = 2, K = 8 on 7 + 5 + 3 frames and a decode pool
of 3 slots on 3, 4, 9 and 1 frames, one stream of which is flushed below 7 frames (the exception's type is printed). One line per output: sha256 of
ids / embeddings / waveform, ``last_status()``, ``library_pushes``, ``launches``, ``fallback_batches``.
"""
import argparse
import hashlib
import os
import statistics
import sys
import time

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--stub", action="store_true", help="recording stubs, no device")
ap.add_argument("--time", action="store_true", help="with --stub: host seconds of the whole script")
ap.add_argument("--reps", type=int, default=15, help="repetitions behind --time")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose audiotoken_amd is used")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
from audiotoken_amd import resample_stream as RS  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.streaming import AcousticDecodeStream, AcousticDecodeStreamPool, AcousticStream, AcousticStreamPool  # noqa: E402

HOP, SR, N_Q = 320, 24000, 4
LINES = []


def say(s: str) -> None:
    LINES.append(s)


def sha(t) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()[:24]


def desc(t) -> str:
    return f"{tuple(t.shape)} {str(t.dtype).replace('torch.', '')} {sha(t)}"


def signal(rng, rate: int, n: int, kind: str, rows: int = 0) -> torch.Tensor:
    """Seeded samples at ``rate``: ``[n]`` (``[rows, n]``), int16 or float32."""
    x = 0.3 * rng.standard_normal((max(rows, 1), n)).astype(np.float32)
    x = torch.from_numpy(np.round(x * 32767.0).clip(-32768, 32767).astype(np.int16) if kind == "int16" else x)
    return x if rows else x[0]


# ---- recording stubs -----------------------------------------------------------------------------------------------------------------------------------
class Stubs:
    """The hooks of one stream or pool. The outputs are a function of the input alone, so that what a stream returns shows what it pushed."""

    def __init__(self, name: str):
        self.name = name

    def encode(self, x, final, started=None):
        say(f"  {self.name}.push_fn {desc(x)} final={final} started={started}")
        assert x.is_contiguous()
        T = -(-x.shape[1] // HOP)
        frames = torch.nn.functional.pad(x, (0, T * HOP - x.shape[1])).reshape(x.shape[0], T, HOP)
        base = (frames.double().sum(-1) * 997.0).round().long()
        return ((base[:, None, :] + torch.arange(N_Q)[None, :, None]) % 1024).to(torch.int16)

    def decode(self, x, started=None):
        say(f"  {self.name}.push_fn {desc(x)} started={started}")
        assert x.is_contiguous()
        return (x.float().mean(1) / 1024.0).repeat_interleave(HOP, dim=-1)

    def gather(self, slots):
        say(f"  {self.name}.gather_fn slots={list(slots)}")

    def scatter(self, slots):
        say(f"  {self.name}.scatter_fn slots={list(slots)}")


def output(label: str, obj, out, resampler=None) -> None:
    outs = sorted(out.items()) if isinstance(out, dict) else [(None, out)]
    what = " ".join((f"{sid}:" if sid is not None else "") + desc(t) for sid, t in outs) or "{}"
    say(f"{label}: {what} frames_emitted={getattr(obj, 'frames_emitted', None)} library_pushes={getattr(obj, 'library_pushes', None)} "
        f"live={getattr(obj, 'live', None)} launches={getattr(resampler, 'launches', None)}")


# ---- --stub: the four classes on stubs -------------------------------------------------------------------------------------------------------------------
ENCODE_PUSHES = (0, 100, 219, 1, 1900, 20, 0, 320, 1927, 5, 2240, 0, 333)      # 319: below a frame; 320 .. 2220: below 7 frames; 2240: across them


def stub_lockstep_encode(rate, kind) -> None:
    name = f"enc[{rate or SR} {kind}]"
    rng = np.random.default_rng(1000 + (rate or 0))
    stubs = Stubs(name)
    rs = RS.HostResampler(SR) if rate else None
    st = AcousticStream(None, 2, push_fn=stubs.encode, n_q=N_Q, sample_rate=rate, resampler=rs)
    scale = (rate or SR) / SR

    def run(tag, pushes, flush=True):
        for i, n in enumerate(pushes):
            output(f"{name} {tag} push {i} n={n}", st, st.push(signal(rng, rate or SR, int(n * scale), kind, rows=2)), rs)
        if flush:
            output(f"{name} {tag} flush", st, st.flush(), rs)
            try:
                st.push(signal(rng, rate or SR, 10, kind, rows=2))
            except RuntimeError as e:
                say(f"{name} {tag} push after flush: {type(e).__name__}: {e}")
    run("a", ENCODE_PUSHES)                         # flush with a held tail
    st.reset()
    run("b", (3000,))                               # reuse
    st.reset()
    run("c", ())                                    # flush with nothing held, before the stream started
    st.reset()
    run("d", (500,))                                # flush before the stream started, with something held
    st.reset()
    run("e", (2240, 640))                           # flush of a started stream with nothing held (at the model's rate)
    st.reset()
    run("f", (700,), flush=False)                   # reset in mid-stream
    st.reset()
    run("g", (2500, 100))


def stub_lockstep_decode() -> None:
    name = "dec"
    rng = np.random.default_rng(2000)
    stubs = Stubs(name)
    st = AcousticDecodeStream(None, 2, push_fn=stubs.decode)

    def run(tag, pushes, K=8, flush=True):
        for i, t in enumerate(pushes):
            output(f"{name} {tag} push {i} t={t}", st, st.push(torch.from_numpy(rng.integers(0, 1024, size=(2, K, t), dtype=np.int64))))
        if flush:
            output(f"{name} {tag} flush", st, st.flush())
            try:
                st.flush()
            except RuntimeError as e:
                say(f"{name} {tag} flush twice: {type(e).__name__}: {e}")
    run("a", (0, 3, 3, 1, 0, 5, 1, 12))             # 6 frames held, the 7th starts the stream; flush with nothing held
    st.reset()
    run("b", (4,))                                  # flush before the stream started
    st.reset()
    run("c", ())
    st.reset()
    run("d", (2, 0), K=2, flush=False)
    st.reset()
    run("e", (9, 1), K=2)


def stub_encode_pool() -> None:
    name = "encpool"
    rng = np.random.default_rng(3000)
    stubs, rs = Stubs(name), RS.HostResampler(SR)
    pool = AcousticStreamPool(None, 4, push_fn=stubs.encode, gather_fn=stubs.gather, scatter_fn=stubs.scatter, n_q=N_Q, resampler=rs)
    fmt = {}
    lengths = (0, 100, 319, 320, 640, 2239, 2240, 2241, 3200, 5000)

    def open_(rate=None, kind="float32"):
        sid = pool.open(sample_rate=rate) if rate else pool.open()
        fmt[sid] = (rate or SR, kind)
        say(f"{name} open -> {sid} rate={rate} live={pool.live}")
        return sid

    def push(tag, sids, ns=None):
        ns = ns if ns is not None else [int(rng.choice(lengths)) for _ in sids]
        items = {sid: signal(rng, fmt[sid][0], n * fmt[sid][0] // SR, fmt[sid][1]) for sid, n in zip(sids, ns)}
        output(f"{name} {tag} push {dict(zip(sids, ns))}", pool, pool.push(items), rs)

    def flush(tag, sids):
        output(f"{name} {tag} flush {sids}", pool, pool.flush(sids), rs)
    a, b, c, d = open_(), open_(16000, "int16"), open_(48000, "float32"), open_()
    push("1", [a, b, c, d], [0, 0, 100, 319])                # nothing goes out
    push("2", [a, b, c, d], [2240, 2240, 2240, 320])         # three start together, one waits
    push("3", [a, b, c, d])
    push("4", [d, b])
    flush("5", b)                                            # a flush in mid-run: its slot is the lowest free one
    e = open_()
    push("6", [a, c, d, e], [640, 640, 641, 2240])           # started and starting groups in one call
    pool.close(a)
    say(f"{name} close {a} live={pool.live}")
    f = open_(16000, "int16")
    push("7", [c, d, e, f])
    push("8", [f, e], [100, 0])
    flush("9", [c, d])                                       # one of them resampled, lengths as they fell
    g, h = open_(48000, "float32"), open_()
    push("10", [e, f, g, h], [3200, 3200, 3200, 3200])
    for i in range(4):
        push(f"11.{i}", [e, f, g, h])
    flush("12", [h])
    flush("13", {e, f, g})
    i_, j = open_(), open_(16000, "int16")
    push("14", [i_, j], [100, 200])
    flush("15", [i_, j])                                     # both before they started
    k = open_()
    flush("16", k)                                           # nothing held at all
    for verb, call in (("push", lambda: pool.push({a: torch.zeros(10)})), ("flush", lambda: pool.flush(99))):
        try:
            call()
        except (RuntimeError, KeyError) as err:
            say(f"{name} {verb} of a stream that is not open: {type(err).__name__}: {err}")


def stub_decode_pool() -> None:
    name = "decpool"
    rng = np.random.default_rng(4000)
    stubs = Stubs(name)
    pool = AcousticDecodeStreamPool(None, 4, push_fn=stubs.decode, gather_fn=stubs.gather, scatter_fn=stubs.scatter)
    K = {}
    lengths = (0, 1, 3, 6, 7, 8, 20)

    def open_(k):
        sid = pool.open()
        K[sid] = k
        say(f"{name} open -> {sid} K={k} live={pool.live}")
        return sid

    def push(tag, sids, ts=None):
        ts = ts if ts is not None else [int(rng.choice(lengths)) for _ in sids]
        items = {sid: torch.from_numpy(rng.integers(0, 1024, size=(K[sid], t), dtype=np.int64)) for sid, t in zip(sids, ts)}
        output(f"{name} {tag} push {dict(zip(sids, ts))}", pool, pool.push(items))

    def flush(tag, sids):
        output(f"{name} {tag} flush {sids}", pool, pool.flush(sids))
    a, b, c, d = open_(8), open_(2), open_(8), open_(2)
    push("1", [a, b, c, d], [0, 3, 6, 6])
    push("2", [a, b, c, d], [7, 4, 1, 1])                    # all start; K = 2 and K = 8 in one call
    push("3", [a, b, c, d])
    push("4", [c, a], [5, 5])
    flush("5", [b])                                          # a started stream holds nothing
    e = open_(8)
    push("6", [a, c, d, e], [3, 3, 3, 9])
    pool.close(c)
    say(f"{name} close {c} live={pool.live}")
    f = open_(2)
    push("7", [a, d, e, f])
    push("8", [f], [4])
    flush("9", [f, a])                                       # whatever they hold, whichever phase they are in
    g = open_(8)
    for i in range(4):
        push(f"10.{i}", [d, e, g])
    flush("11", {d, e, g})
    h = open_(8)
    flush("12", h)


def stub_script() -> None:
    stub_lockstep_encode(None, "float32")
    stub_lockstep_encode(16000, "int16")
    stub_lockstep_encode(48000, "float32")
    stub_lockstep_decode()
    stub_encode_pool()
    stub_decode_pool()


# ---- default: the real models ---------------------------------------------------------------------------------------------------------------------------
def device_line(label: str, model, obj, resampler=None, **tensors) -> None:
    status = model.last_status()   # synchronises
    say(f"{label}: " + " ".join(f"{k}={sha(v)}" for k, v in tensors.items()) + f" status={status} library_pushes={getattr(obj, 'library_pushes', None)} "
        f"launches={getattr(resampler, 'launches', None)} fallback_batches={obj.fallback_batches}")


def device_script() -> None:
    from audiotoken_amd.configs import AcousticDecoderConfig, AcousticEncoderConfig
    from audiotoken_amd.decoder import AcousticDecoder
    from audiotoken_amd.encoder import AcousticEncoder
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    rs = enc.resampler()
    wav = torch.from_numpy(W.synth_waveform(3, 6440, SR, seed=7999)).cuda()
    st = enc.new_stream(batch=3)
    st.keep_embeddings = True
    at = 0
    for i, n in enumerate((2240, 3200, 1000)):
        ids = st.push(wav[:, at:at + n]) if i < 2 else torch.cat([st.push(wav[:, at:at + n]), st.flush()], dim=-1)
        at += n
        device_line(f"encode stream push {i} n={n}", enc, st, ids=ids, emb=st.last_embeddings)
    wav16 = torch.from_numpy(W.synth_waveform(3, 6440 * 2 // 3, 16000, seed=7999)).cuda()
    st = enc.new_stream(batch=3, sample_rate=16000)
    at = 0
    for i, n in enumerate((1493, 2133, 667)):
        device_line(f"encode stream 16 kHz push {i} n={n}", enc, st, rs, ids=st.push(wav16[:, at:at + n]))
        at += n
    device_line("encode stream 16 kHz flush", enc, st, rs, ids=st.flush())

    rng = np.random.default_rng(5000)
    clips = torch.from_numpy(W.synth_waveform(5, 12000, SR, seed=7100)).cuda()
    pool = enc.new_stream_pool(4)
    pos = {}

    def feed(tag, sids):
        items = {}
        for sid in sids:
            n = int(rng.integers(100, 4001))
            items[sid] = clips[sid % 5, pos[sid]:pos[sid] + n]
            pos[sid] += n
        out = pool.push(items)
        device_line(f"encode pool {tag} push {[int(v.shape[0]) for v in items.values()]}", enc, pool, **{f"ids{sid}": out[sid] for sid in sorted(out)})
    first = [pool.open() for _ in range(3)]
    pos.update({sid: 0 for sid in first})
    feed("1", first)
    feed("2", first)
    late = pool.open()                      # opened after the others started
    pos[late] = 0
    for i in range(3, 7):
        feed(str(i), first + [late])
    pool.close(first[1])
    rest = [first[0], first[2], late]
    feed("7", rest)
    out = pool.flush(rest)
    device_line(f"encode pool flush {rest}", enc, pool, **{f"ids{sid}": out[sid] for sid in sorted(out)})
    del enc, pool, st
    torch.cuda.empty_cache()

    dec = AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=True))
    tok = torch.from_numpy(np.random.default_rng(8999).integers(0, W.ENCODEC_CODEBOOK, size=(4, 8, 17), dtype=np.int64)).cuda()
    st = dec.new_stream(batch=2)
    at = 0
    for i, t in enumerate((7, 5, 3)):
        device_line(f"decode stream push {i} t={t}", dec, st, wav=st.push(tok[:2, :, at:at + t]))
        at += t
    device_line("decode stream flush", dec, st, wav=st.flush())
    pool = dec.new_stream_pool(3)
    a, b, c = pool.open(), pool.open(), pool.open()
    at = 0
    for i, t in enumerate((3, 4, 9, 1)):
        live = pool.live
        out = pool.push({sid: tok[sid % 4, :, at:at + t] for sid in live})
        device_line(f"decode pool push {i} t={t} live={live}", dec, pool, **{f"wav{sid}": out[sid] for sid in sorted(out)})
        at += t
        if i == 0:                          # 3 frames in all: the library refuses them as it refuses a one-shot decode of T = 3
            try:
                pool.flush(c)
                say("decode pool flush below 7 frames: no exception")
            except Exception as e:   # noqa: BLE001 — the type is what is listed
                say(f"decode pool flush below 7 frames: {type(e).__name__} live={pool.live}")
    out = pool.flush([a, b])
    device_line("decode pool flush", dec, pool, **{f"wav{sid}": out[sid] for sid in sorted(out)})


if __name__ == "__main__":
    if args.stub:
        stub_script()
        print("\n".join(LINES), flush=True)
        if args.time:
            secs = []
            for _ in range(args.reps):
                LINES.clear()
                t0 = time.perf_counter()
                stub_script()
                secs.append(time.perf_counter() - t0)
            print(f"host seconds of the stub script: median of {args.reps} = {statistics.median(secs):.4f} [{min(secs):.4f} .. {max(secs):.4f}]")
    else:
        assert torch.cuda.is_available(), "needs a HIP device (or --stub)"
        device_script()
        print("\n".join(LINES), flush=True)
