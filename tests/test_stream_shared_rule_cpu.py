"""The residual buffering of a lockstep stream and of a pool is ONE rule (audiotoken_amd/streaming.py): a lockstep stream of batch 1 and a pool of one
slot, fed the same pushes, hand the library the same calls — shape, content, ``final``, ``started`` — and return the same output. On stubs, for encode,
for decode, and for encode at a sample rate of its own on ``HostResampler``; 200 seeded schedules each, with zero-length pushes and totals below the
7 frames a stream needs to start among them."""
import numpy as np
import pytest
import torch

from audiotoken_amd import resample_stream as RS
from audiotoken_amd.streaming import (FIRST_PUSH_FRAMES, HOP, SAMPLE_RATE, AcousticDecodeStream, AcousticDecodeStreamPool, AcousticStream,
                                      AcousticStreamPool)

SCHEDULES = 200
N_Q = 4


class _Library:
    """The stub behind a stream: records every call and answers with a function of the input alone."""

    def __init__(self):
        self.calls = []

    def _record(self, x, final, started):
        assert x.is_contiguous()
        # the lockstep hooks are not told `started`: a stream has started when the library has seen a push of it
        self.calls.append((tuple(x.shape), x.dtype, x.clone(), final, bool(self.calls) if started is None else started))

    def encode(self, x, final, started=None):
        self._record(x, final, started)
        T = -(-x.shape[1] // HOP)
        frames = torch.nn.functional.pad(x, (0, T * HOP - x.shape[1])).reshape(x.shape[0], T, HOP)
        base = (frames.double().sum(-1) * 997.0).round().long()
        return ((base[:, None, :] + torch.arange(N_Q)[None, :, None]) % 1024).to(torch.int16)

    def decode(self, x, started=None):
        self._record(x, None, started)
        return (x.float().mean(1) / 1024.0).repeat_interleave(HOP, dim=-1)


def _same_calls(a: _Library, b: _Library, what: str) -> None:
    assert len(a.calls) == len(b.calls), f"{what}: {len(a.calls)} library calls of the stream, {len(b.calls)} of the pool"
    for i, (ca, cb) in enumerate(zip(a.calls, b.calls)):
        assert ca[0] == cb[0] and ca[1] == cb[1] and ca[3:] == cb[3:], f"{what}, call {i}: {ca[:2] + ca[3:]} != {cb[:2] + cb[3:]}"
        assert torch.equal(ca[2], cb[2]), f"{what}, call {i}: the content differs"


def _lengths(rng, unit: int, s: int) -> list:
    """The pushes of schedule ``s`` in items: every fourth schedule stays below the first push's minimum in total, and zero-length pushes are everywhere."""
    small = s % 4 == 0
    count = int(rng.integers(0, 9))
    top = (FIRST_PUSH_FRAMES * unit - 1) // max(count, 1) if small else 12 * unit
    out = [int(rng.choice((0, 1, unit - 1, unit, unit + 1, int(rng.integers(0, top + 1)), int(rng.integers(0, top + 1))))) for _ in range(count)]
    out = [min(n, top) for n in out]
    assert not small or sum(out) < FIRST_PUSH_FRAMES * unit
    return out


def _run_pair(stream, pool, sid, pieces, what):
    """Push ``pieces`` ([1, ..., n] each) through both, flush both; the concatenated outputs."""
    got_s, got_p = [], []
    for x in pieces:
        got_s.append(stream.push(x)[0])
        got_p.append(pool.push({sid: x[0]})[sid])
    got_s.append(stream.flush()[0])
    got_p.append(pool.flush(sid)[sid])
    for i, (a, b) in enumerate(zip(got_s, got_p)):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), f"{what}: output {i} differs"
    assert pool.live == []
    return torch.cat(got_s, dim=-1), torch.cat(got_p, dim=-1)


@pytest.mark.parametrize("rate", [None, 16000])
def test_encode_stream_and_one_slot_pool_are_one_rule(rate):
    totals = []
    for s in range(SCHEDULES):
        rng = np.random.default_rng(100_000 * (rate or 1) + s)
        lib_s, lib_p = _Library(), _Library()
        stream = AcousticStream(None, 1, push_fn=lib_s.encode, n_q=N_Q, sample_rate=rate, resampler=RS.HostResampler(SAMPLE_RATE) if rate else None)
        pool = AcousticStreamPool(None, 1, push_fn=lib_p.encode, gather_fn=lambda slots: None, scatter_fn=lambda slots: None, n_q=N_Q,
                                  resampler=RS.HostResampler(SAMPLE_RATE) if rate else None)
        sid = pool.open(sample_rate=rate) if rate else pool.open()
        ns = [n * rate // SAMPLE_RATE for n in _lengths(rng, HOP, s)] if rate else _lengths(rng, HOP, s)
        if rate and s % 2:
            pieces = [torch.from_numpy(rng.integers(-20000, 20000, size=(1, n)).astype(np.int16)) for n in ns]
        else:
            pieces = [torch.from_numpy(0.3 * rng.standard_normal((1, n)).astype(np.float32)) for n in ns]
        a, b = _run_pair(stream, pool, sid, pieces, f"schedule {s} {ns}")
        _same_calls(lib_s, lib_p, f"schedule {s} {ns}")
        assert torch.equal(a, b) and a.shape[-1] == stream.frames_emitted
        assert pool.library_pushes == len(lib_p.calls)
        totals.append(sum(ns) * (SAMPLE_RATE / rate if rate else 1))
    assert min(totals) == 0 and sum(t < FIRST_PUSH_FRAMES * HOP for t in totals) >= SCHEDULES // 4 and max(totals) > 20 * HOP   # the schedules are what they claim


def test_decode_stream_and_one_slot_pool_are_one_rule():
    totals = []
    for s in range(SCHEDULES):
        rng = np.random.default_rng(300_000 + s)
        K = (2, 8)[s % 2]
        lib_s, lib_p = _Library(), _Library()
        stream = AcousticDecodeStream(None, 1, push_fn=lib_s.decode)
        pool = AcousticDecodeStreamPool(None, 1, push_fn=lib_p.decode, gather_fn=lambda slots: None, scatter_fn=lambda slots: None)
        sid = pool.open()
        ts = _lengths(rng, 1, s)
        pieces = [torch.from_numpy(rng.integers(0, 1024, size=(1, K, t), dtype=np.int64)) for t in ts]
        a, b = _run_pair(stream, pool, sid, pieces, f"schedule {s} K={K} {ts}")
        _same_calls(lib_s, lib_p, f"schedule {s} K={K} {ts}")
        assert torch.equal(a, b) and a.shape[-1] == HOP * stream.frames_emitted == HOP * sum(ts)
        totals.append(sum(ts))
    assert min(totals) == 0 and sum(t < FIRST_PUSH_FRAMES for t in totals) >= SCHEDULES // 4 and max(totals) > 20
