"""Streaming acoustic encode and decode: audio (tokens) pushed in pieces, the tokens (audio) of the whole
(``at_encodec_encode_stream_checked`` / ``at_encodec_decode_stream_checked``).

``AcousticEncoder.new_stream(batch)`` returns an :class:`AcousticStream`. After any sequence of ``push`` calls and one ``flush`` the
concatenated tokens are the tokens one-shot ``encode`` gives for the concatenated audio, in memory bounded by the largest push.
``AcousticDecoder.new_stream(batch)`` returns an :class:`AcousticDecodeStream`, the way back: tokens pushed frame by frame, the waveform one-shot
``decode`` gives for the concatenated tokens, 320 samples per frame as they arrive. ``new_stream_pool(slots)`` of either returns a pool
(:class:`AcousticStreamPool`, :class:`AcousticDecodeStreamPool`): streams that start and finish on their own, batched per call by phase and length
(DESIGN.md section 15).

The four classes are one contract, and every rule of it is written once, here:

* a DIRECTION (``_ENCODE``, ``_DECODE``) says what differs between the two ways: the unit along the time axis (320 samples or 1 frame), the input
  dtype, the empty output, the texts, the library's entry points and the bare ``*_stream_checked`` push on a pair of state buffers;
* the RESIDUAL BUFFERING (``_ready``, ``_split``): along the last axis, what does not fill a unit is held, a stream that has not started waits for
  ``FIRST_PUSH_FRAMES`` units, ``flush`` sends what is held. The axes in front (batch, codebooks) are carried along;
* the TRANSACTION: the bare push, then ``fallback.encodec_ladder`` repeating it from the untouched input state, then commit. A lockstep stream
  (``_Stream``) commits by swapping its two state buffers; a pool (``_StreamPool``) gathers its rows into a staging state, pushes staging-in ->
  staging-out and scatters back;
* the RESAMPLE PRELUDE (``_resample``): streams with a sample rate of their own turn what they were pushed into samples at the model's rate, all
  streams of a call in one launch, before any of it reaches the library (resample_stream.py).
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Tuple, Union

import torch

from . import _cabi, fallback
from . import resample_stream as RS
from . import weights as W

HOP = W.ENCODEC_HOP          # 320 samples per frame
FIRST_PUSH_FRAMES = 7        # the library's minimum for the first push of a stream (include/audiotoken_hip.h)
SAMPLE_RATE = 24_000         # EnCodec's rate: what a stream without an encoder (push_fn) resamples to


# ======================================================================================================================================================
# The two directions
# ======================================================================================================================================================
@dataclass(frozen=True)
class _Direction:
    unit: int                 # items along the last axis per frame
    dtype: torch.dtype        # what the pushed items are cast to
    noun: str                 # the pushed items in messages ...
    axes: str                 # ... and the axes of one stream's items (the last one is time) ...
    ndim: int                 # ... counted
    has_final: bool           # whether the library's push is told that it is the last one. Decode has no such flag: its flush is a push like any other
    nonfinite_bit: bool       # whether the call has a quantiser (status bit 2), for the ladder
    what: str                 # noun of the ladder's log lines: a lockstep push ...
    pool_what: str            # ... and a pool's
    empty: Callable           # (leading shape, n_q, device) -> the output of a call that pushed nothing
    call: Callable            # (model, state_in, state_out, x, final, n_q, keep_embeddings) -> (output, embeddings or None): the bare library push
    state_bytes: Callable     # lib -> the entry point; also below
    reset: Callable
    gather: Callable
    scatter: Callable


def _encode_call(enc, state_in, state_out, x, final, n_q, keep_embeddings):
    lib = enc._h.lib
    B, n = x.shape
    T = -(-n // HOP)
    codes = torch.empty((B, n_q, T), dtype=torch.int16, device=enc.device)
    emb = torch.empty((B, T, W.ENCODEC_DIM), dtype=torch.float32, device=enc.device) if keep_embeddings else None
    nbytes = lib.at_encodec_stream_workspace_bytes(enc._h.handle, B, n)
    ws = enc._workspace(nbytes)
    t_out = C.c_int(0)
    with torch.cuda.device(enc.device):
        rc = lib.at_encodec_encode_stream_checked(enc._h.handle, state_in.data_ptr(), state_out.data_ptr(), x.data_ptr(), B, n, 1 if final else 0, n_q,
                                                  codes.data_ptr(), C.byref(t_out), _cabi.ptr(emb), ws.data_ptr(), nbytes,
                                                  _cabi.current_stream_handle(enc.device), enc._status.data_ptr())
    _cabi.check(rc, "at_encodec_encode_stream_checked")
    assert t_out.value == T, (t_out.value, T)
    return codes, emb


def _decode_call(dec, state_in, state_out, codes, final, n_q, keep_embeddings):
    lib = dec._h.lib
    B, K, t = codes.shape
    wav = torch.empty((B, HOP * t), dtype=torch.float32, device=dec.device)
    nbytes = lib.at_encodec_decode_stream_workspace_bytes(dec._h.handle, B, t)
    ws = dec._workspace(nbytes)
    with torch.cuda.device(dec.device):
        rc = lib.at_encodec_decode_stream_checked(dec._h.handle, state_in.data_ptr(), state_out.data_ptr(), codes.data_ptr(), B, K, t, wav.data_ptr(),
                                                  ws.data_ptr(), nbytes, _cabi.current_stream_handle(dec.device), dec._status.data_ptr())
    _cabi.check(rc, "at_encodec_decode_stream_checked")
    return wav, None


_ENCODE = _Direction(
    unit=HOP, dtype=torch.float32, noun="samples", axes="n", ndim=1, has_final=True, nonfinite_bit=True,
    what="acoustic stream push", pool_what="acoustic stream pool push",
    empty=lambda lead, n_q, device: torch.empty((*lead, n_q, 0), dtype=torch.int16, device=device), call=_encode_call,
    state_bytes=lambda lib: lib.at_encodec_stream_state_bytes, reset=lambda lib: lib.at_encodec_stream_reset,
    gather=lambda lib: lib.at_encodec_stream_gather, scatter=lambda lib: lib.at_encodec_stream_scatter)

_DECODE = _Direction(
    unit=1, dtype=torch.long, noun="tokens", axes="K, t", ndim=2, has_final=False, nonfinite_bit=False,
    what="acoustic decode stream push", pool_what="acoustic decode stream pool push",
    empty=lambda lead, n_q, device: torch.empty((*lead, 0), dtype=torch.float32, device=device), call=_decode_call,
    state_bytes=lambda lib: lib.at_encodec_decode_stream_state_bytes, reset=lambda lib: lib.at_encodec_decode_stream_reset,
    gather=lambda lib: lib.at_encodec_decode_stream_gather, scatter=lambda lib: lib.at_encodec_decode_stream_scatter)


def _new_states(d: _Direction, model, B: int, count: int) -> List[torch.Tensor]:
    """``count`` uninitialised state buffers for ``B`` streams (a state of fewer streams is the first ``state_bytes`` of it)."""
    nbytes = d.state_bytes(model._h.lib)(model._h.handle, B)
    return [torch.empty(nbytes, dtype=torch.uint8, device=model.device) for _ in range(count)]


def _reset(d: _Direction, model, state: torch.Tensor, B: int) -> None:
    """``state`` becomes the state of ``B`` streams that have not started (h = c = 0, true left reflect padding)."""
    fn = d.reset(model._h.lib)
    with torch.cuda.device(model.device):
        rc = fn(model._h.handle, state.data_ptr(), B, _cabi.current_stream_handle(model.device))
    _cabi.check(rc, fn.__name__)


def _hook(d: _Direction, push_fn: Callable) -> Callable:
    """A ``push_fn`` stub as it is called in here, ``(x, final[, started])``: the stubs of a direction without a final push do not take ``final``."""
    return push_fn if d.has_final else (lambda x, final, *started: push_fn(x, *started))


# ======================================================================================================================================================
# The residual buffering and the resample prelude
# ======================================================================================================================================================
def _ready(n_held: int, unit: int, started: bool) -> int:
    """THE buffering rule: of ``n_held`` items, how many go to the library now. Whole units only, and none before a stream that has not started
    holds ``FIRST_PUSH_FRAMES`` of them."""
    n = n_held // unit * unit
    return 0 if not started and n < FIRST_PUSH_FRAMES * unit else n


def _cat(held: Optional[torch.Tensor], new: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return new if held is None else held if new is None else torch.cat([held, new], dim=-1)


def _split(held: Optional[torch.Tensor], new: Optional[torch.Tensor], unit: int, started: bool) -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """``new`` after ``held`` along the last axis -> ``(what goes to the library, what is held on)``; None where that is nothing."""
    x = _cat(held, new)
    total = 0 if x is None else x.shape[-1]
    n = _ready(total, unit, started)
    rest = x[..., n:] if n < total else None
    if rest is not None and held is None:   # `x` is the caller's tensor, not a concatenation made here: hold a copy of its end, not a view of it
        rest = rest.clone()
    return (x[..., :n] if n else None), rest


def _rate_state(model, sample_rate: int, batch: int, resampler):
    """``(RateState, resampler)`` of a stream that is pushed raw samples at ``sample_rate``; the resampler is the model's unless one is given."""
    model_rate = model.config.model_sample_rate if model is not None else SAMPLE_RATE
    rate = RS.RateState(sample_rate, model_rate, batch)
    if resampler is None:
        resampler = model.resampler() if model is not None else RS.HostResampler(model_rate)
    return rate, resampler


def _resample(resampler, entries: List[Tuple[RS.RateState, Optional[torch.Tensor]]], final: bool, device) -> List[List[torch.Tensor]]:
    """Raw samples ``[B, n]`` at each entry's rate (None: none, the flush) -> what they add to the signal at the model's rate, per entry its ``B`` rows
    ``float32 [m]``. ONE launch for all entries; their source tails move on, so the caller puts the result into ``held`` at once, where it outlives a
    push of the library that fails."""
    todo, jobs = [], []
    for rate, x in entries:
        window, n_new = rate.window(x, device)
        plan = RS.plan_push(rate.pos, n_new, final)
        todo.append((rate, window, plan))
        jobs.extend(rate.jobs(window, plan))
    outs = resampler.run(jobs) if any(j.plan.out_len for j in jobs) else [j.pcm.new_zeros(0, dtype=torch.float32) for j in jobs]
    res, at = [], 0
    for rate, window, plan in todo:
        rate.advance(window, plan)
        res.append(outs[at:at + rate.batch])
        at += rate.batch
    return res


# ======================================================================================================================================================
# Lockstep streams: all rows of the batch advance together
# ======================================================================================================================================================
class _Stream:
    """What the two lockstep streams share, which is everything but the direction ``_DIR``, the constructor's arguments and the name under which each
    keeps its model (``_enc``, ``_dec``; ``_model`` here).

    A push is a transaction: the library reads ``_state[0]`` and writes ``_state[1]``; the status word is read once (one synchronisation), a non-zero
    one repeats the push from the untouched input state by ``fallback.encodec_ladder``, and the two buffers change places when it succeeded. ``push_fn``
    replaces the whole transaction (the host-side buffering is tested with a stub). Decode has no codebooks to choose and no embedding tap: ``n_q``,
    ``keep_embeddings`` and ``last_embeddings`` stay as they are here."""
    _DIR: _Direction
    n_q = None
    keep_embeddings = False
    last_embeddings: Optional[torch.Tensor] = None
    _rate = None

    def __init__(self, batch: int, push_fn: Optional[Callable]):
        assert batch >= 1, "batch must be >= 1"
        model = self._model
        self.batch = int(batch)
        self._device = model.device if model is not None else torch.device("cpu")
        self._push_fn = _hook(self._DIR, push_fn) if push_fn is not None else self._device_push
        self._state = _new_states(self._DIR, model, self.batch, 2) if push_fn is None else None
        self.reset()

    def reset(self) -> None:
        """Forget everything: the next push starts a new stream (h = c = 0, true left reflect padding)."""
        self._held: Optional[torch.Tensor] = None   # [B, ..., t]: items that do not fill a frame, or the first push's minimum, yet
        self._started = False
        self._finished = False
        self.frames_emitted = 0
        if self._rate is not None:
            self._rate.reset()
        if self._state is not None:
            _reset(self._DIR, self._model, self._state[0], self.batch)

    @property
    def fallback_batches(self) -> int:
        return self._model.fallback_batches if self._model is not None else 0

    def _not_finished(self, verb: str) -> None:
        if self._finished:
            raise RuntimeError(f"{type(self).__name__}: {verb}; call reset() to start a new stream")

    def _hold_resampled(self, samples, final: bool) -> None:
        rows, = _resample(self._resampler, [(self._rate, samples)], final, self._device)
        self._held = _cat(self._held, torch.stack(rows))

    def _emit(self, piece: Optional[torch.Tensor], final: bool) -> torch.Tensor:
        self.last_embeddings = None
        if piece is None:
            return self._DIR.empty((self.batch,), self.n_q, self._device)
        out = self._push_fn(piece.contiguous(), final and self._DIR.has_final)
        self.frames_emitted += -(-piece.shape[-1] // self._DIR.unit)
        return out

    def push(self, x: torch.Tensor) -> torch.Tensor:
        d = self._DIR
        self._not_finished("push after flush()")
        if self._rate is not None:
            self._hold_resampled(x, False)
            x = None
        else:
            assert x.dim() == 1 + d.ndim and x.shape[0] == self.batch, f"{d.noun} must be [{self.batch}, {d.axes}]"
            if self._model is not None:
                x = x.to(device=self._device, dtype=d.dtype)
        piece, rest = _split(self._held, x, d.unit, self._started)
        out = self._emit(piece, False)
        self._held = rest        # only now: the push succeeded
        self._started = self._started or piece is not None
        return out

    def flush(self) -> torch.Tensor:
        """What is held goes out (encode: with the one-shot path's right-edge padding). The stream is finished afterwards."""
        self._not_finished("flush() twice")
        if self._rate is not None:
            self._hold_resampled(None, True)
        held, self._held, self._finished = self._held, None, True
        return self._emit(held if held is not None and held.shape[-1] else None, True)

    # ---- device side: one transaction -------------------------------------------------------------------------------------------
    def _call(self, x: torch.Tensor, final: bool) -> torch.Tensor:
        """The bare library push, ``_state[0]`` -> ``_state[1]``."""
        out, self.last_embeddings = self._DIR.call(self._model, self._state[0], self._state[1], x, final, self.n_q, self.keep_embeddings)
        return out

    def _device_push(self, x: torch.Tensor, final: bool = False) -> torch.Tensor:
        d, m = self._DIR, self._model
        # every repeat starts from the same input state: a failed call wrote the other buffer only
        out = fallback.encodec_ladder(m, self._call(x, final), lambda: self._call(x, final), self.batch, m.RANGE_OPTIONS, d.what, nonfinite_bit=d.nonfinite_bit)
        self._state.reverse()   # success: the written buffer is the next push's input
        return out


class AcousticStream(_Stream):
    """``push(samples [B, n]) -> int16 [B, n_q, t]`` on the device (``t`` may be 0), ``flush() -> int16 [B, n_q, t_last]``, ``reset()``.

    All ``batch`` rows advance in lockstep. What does not fill a frame is held, the first push waits for 7 frames, and ``flush`` sends the rest with the
    one-shot path's right-edge padding. When the device status word of a push is non-zero the push is repeated on the safe kernels, by the ladder
    ``AcousticEncoder.verified`` repeats a batch with (audiotoken_amd/fallback.py; bit 1: this push on the bf16x3 kernels, counted in
    ``fallback_batches``, the next push on f16x2 again; bit 0: the LSTM route is switched for the rest of the handle's life).

    ``push_fn(samples [B, n], final) -> codes [B, n_q, t]`` replaces the device call. ``keep_embeddings``: a parity tap; when set, every library push
    also leaves its pre-quantiser embedding ``[B, t, 128]`` in ``last_embeddings`` (None after a call that pushed nothing).

    ``sample_rate``: the stream takes RAW samples at that rate (float32 or int16, torch or numpy) and resamples them on the device at stream-global
    positions, carrying the source tail across pushes (resample_stream.py): the tokens are those of the whole signal resampled
    once. The resampled samples enter the residual buffering like pushed ones. None: samples are float at the model's rate, as ever.
    """
    _DIR = _ENCODE
    _model = property(lambda self: self._enc)

    def __init__(self, encoder=None, batch: int = 1, push_fn: Optional[Callable] = None, n_q: Optional[int] = None, sample_rate: Optional[int] = None,
                 resampler=None):
        if sample_rate is not None:
            self._rate, self._resampler = _rate_state(encoder, sample_rate, int(batch), resampler)
        self.n_q = int(n_q if n_q is not None else encoder.n_q)
        self._enc = encoder
        super().__init__(batch, push_fn)


class AcousticDecodeStream(_Stream):
    """``push(tokens [B, K, t]) -> float32 [B, 320 * t']`` on the device, ``flush()``, ``reset()``.

    ``t'`` is ``t`` once the stream has started; before that, tokens are held until ``FIRST_PUSH_FRAMES`` frames are there (``t' = 0``) and then go
    out together: the first device push is a one-shot decode of its frames, whose left reflect padding needs 7 of them. ``flush()`` decodes what is
    still held, which only happens when the stream never started; with fewer than 7 frames in total it raises what one-shot decode raises for that
    ``T``. A started stream holds nothing, so its ``flush()`` returns ``[B, 0]``. The ladder runs with ``AcousticDecoder.RANGE_OPTIONS``.

    ``push_fn(tokens [B, K, t]) -> wav [B, 320 * t]`` replaces the device call.
    """
    _DIR = _DECODE
    _model = property(lambda self: self._dec)

    def __init__(self, decoder=None, batch: int = 1, push_fn: Optional[Callable] = None):
        self._dec = decoder
        super().__init__(batch, push_fn)


# ======================================================================================================================================================
# Stream pools: the rows of a push still advance in lockstep, but WHICH streams form the rows changes from call to call
# ======================================================================================================================================================
class _Row:
    """Host-side record of one open stream of a pool."""
    __slots__ = ("slot", "held", "started", "rate")

    def __init__(self, slot: int):
        self.slot = slot
        self.rate = None                           # encode: resample_stream.RateState of a stream opened with a sample rate of its own
        self.held: Optional[torch.Tensor] = None   # what the buffering rule holds: samples [n] or tokens [K, t]
        self.started = False


class _StreamPool:
    """What the two pools share, which is everything but the direction ``_DIR`` and the constructor's arguments.

    Every stream is buffered like a lockstep stream of its own. Its device state lives in row ``slot`` of a pool state for ``slots`` streams. One
    GROUP — ids of one call in the same phase whose pieces have the same shape — is one library push of ``B = len(group)`` on two staging states:
    ``gather`` (pool -> staging_in; a starting group resets staging_in instead), the unchanged lockstep push staging_in -> staging_out with its status
    word read once and ``fallback.encodec_ladder`` repeating it from staging_in when it is non-zero, and only then ``scatter`` (staging_out -> pool; not
    after a final push, whose slots are free). A failed push never reaches the pool, nor the rows' ``held`` and ``started``.

    ``push_fn``, ``gather_fn(slots)`` and ``scatter_fn(slots)`` replace the three device calls (``push_fn`` is the BARE library push, which also gets
    ``started``); ``owner`` is then what the ladder reads the status from (None: no status, no repeats). The bookkeeping is tested on the CPU that way.
    """
    _DIR: _Direction
    n_q = None
    keep_embeddings = False
    _resampler = None

    def __init__(self, model=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None):
        assert slots >= 1, "slots must be >= 1"
        assert (push_fn is None) == (gather_fn is None) == (scatter_fn is None), "push_fn, gather_fn and scatter_fn replace the device calls together"
        self._model = model
        self.slots = int(slots)
        self._device = model.device if model is not None else torch.device("cpu")
        self._rows: Dict[int, _Row] = {}
        self._free: List[int] = list(range(self.slots))
        self._next_id = 0
        self.library_pushes = 0    # groups pushed: one library push each (repeats of a failed push not counted)
        self.last_embeddings: Dict[int, torch.Tensor] = {}
        self._emb = None
        self._push = _hook(self._DIR, push_fn) if push_fn is not None else self._device_call
        self._gather = gather_fn if gather_fn is not None else (lambda slots: self._device_copy(True, slots))
        self._scatter = scatter_fn if scatter_fn is not None else (lambda slots: self._device_copy(False, slots))
        self._owner = model if push_fn is None else owner
        self._pool = self._staging = None
        if push_fn is None:
            # the pool and two staging states, each large enough for every slot at once
            self._pool, *self._staging = _new_states(self._DIR, model, self.slots, 3)
            _reset(self._DIR, model, self._pool, self.slots)

    # ---- ids and slots ----------------------------------------------------------------------------------------------------------------------------
    @property
    def live(self) -> List[int]:
        return sorted(self._rows)

    @property
    def fallback_batches(self) -> int:
        return self._owner.fallback_batches if self._owner is not None else 0

    def open(self) -> int:
        """A new stream in the lowest free slot; its id (ids are never reused)."""
        if not self._free:
            raise RuntimeError(f"{type(self).__name__}: all {self.slots} slots are in use; flush() or close() a stream first")
        sid = self._next_id
        self._next_id += 1
        self._rows[sid] = _Row(self._free.pop(0))
        return sid

    def close(self, sid: int) -> None:
        """Drop a stream without output; its slot is free (the slot's rows are overwritten when its next stream is first scattered)."""
        self._release(self._row(sid, "close"), sid)

    def _release(self, row: _Row, sid: int) -> None:
        del self._rows[sid]
        self._free.append(row.slot)
        self._free.sort()

    def _row(self, sid: int, verb: str) -> _Row:
        row = self._rows.get(sid)
        if row is None:
            if isinstance(sid, int) and 0 <= sid < self._next_id:   # ids are never reused: this one was flushed or closed
                raise RuntimeError(f"{type(self).__name__}: {verb} after flush() or close() of stream {sid}; open() a new one")
            raise KeyError(f"{type(self).__name__}: no stream {sid} (open() returns the ids)")
        return row

    # ---- push and flush -------------------------------------------------------------------------------------------------------------------------------
    def _hold_resampled(self, rows: Dict[int, _Row], items: Dict[int, Optional[torch.Tensor]], final: bool) -> None:
        """The rows with a rate of their own: ONE launch turns what they were pushed into samples at the model's rate, which go into ``held`` at once."""
        todo = []
        for sid, row in rows.items():
            if row.rate is not None:
                x = items[sid]
                if x is not None:
                    x = RS.as_pcm(x)
                    assert x.dim() == 1, "samples of a stream must be [n]"
                    x = x[None]
                todo.append((row, x))
        if todo:
            outs = _resample(self._resampler, [(row.rate, x) for row, x in todo], final, self._device)
            for (row, _), (y,) in zip(todo, outs):
                row.held = _cat(row.held, y)

    def push(self, items: Dict[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
        d = self._DIR
        rows = {sid: self._row(sid, "push") for sid in sorted(items)}
        self._hold_resampled(rows, items, False)
        ready = {}
        for sid, row in rows.items():
            x = None
            if row.rate is None:
                x = items[sid]
                assert x.dim() == d.ndim, f"{d.noun} of a stream must be [{d.axes}]"
                if self._model is not None:
                    x = x.to(device=self._device, dtype=d.dtype)
            ready[sid] = _split(row.held, x, d.unit, row.started)
        return self._run_groups(ready, False)

    def flush(self, sids: Union[int, Iterable[int]]) -> Dict[int, torch.Tensor]:
        """What these streams hold goes out (encode: with the one-shot path's right-edge padding; decode: streams that never reached 7 frames, which
        the library refuses as it refuses a one-shot decode of that T). Their slots are free afterwards."""
        sids = [sids] if isinstance(sids, int) else sorted(set(sids))
        rows = {sid: self._row(sid, "flush") for sid in sids}
        self._hold_resampled(rows, dict.fromkeys(rows), True)
        try:
            return self._run_groups({sid: (row.held if row.held is not None and row.held.shape[-1] else None, None) for sid, row in rows.items()}, True)
        finally:   # finished, whatever the library said about a clip below its minimum
            for sid, row in rows.items():
                self._release(row, sid)

    def _run_groups(self, ready: Dict[int, Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]], final: bool) -> Dict[int, torch.Tensor]:
        """``{sid: (piece for the library or None, what the stream holds afterwards)}`` -> ``{sid: output}``. Streams in the same phase with pieces of the
        same shape share one transaction; the groups run by ascending smallest id, ids ascending inside a group, and a group's rows move on when its
        push succeeded."""
        d = self._DIR
        final = final and d.has_final
        out: Dict[int, torch.Tensor] = {}
        self.last_embeddings = {}
        groups: Dict[tuple, List[int]] = {}
        for sid in sorted(ready):
            piece, rest = ready[sid]
            if piece is None:
                self._rows[sid].held = rest
                out[sid] = d.empty((), self.n_q, self._device)
            else:
                groups.setdefault((self._rows[sid].started, tuple(piece.shape)), []).append(sid)
        for (started, _), ids in sorted(groups.items(), key=lambda g: g[1][0]):
            self._run(ids, [ready[i][0] for i in ids], started, final, out)
            for sid in ids:
                self._rows[sid].held, self._rows[sid].started = ready[sid][1], True
        return out

    def _run(self, ids: List[int], xs: List[torch.Tensor], started: bool, final: bool, out: Dict[int, torch.Tensor]) -> None:
        """One group: the pieces ``xs`` of the streams ``ids`` as the rows of one transaction, its output rows into ``out``."""
        x = torch.stack(xs).contiguous()
        res = self._transaction([self._rows[i].slot for i in ids], started, final, lambda: self._push(x, final, started))
        for b, sid in enumerate(ids):
            out[sid] = res[b]
            if self._emb is not None:
                self.last_embeddings[sid] = self._emb[b]
        self._emb = None

    # ---- one group = one transaction ------------------------------------------------------------------------------------------------------------------
    def _transaction(self, slots: List[int], started: bool, final: bool, call: Callable):
        B = len(slots)
        if started:
            self._gather(slots)
        elif self._staging is not None:
            _reset(self._DIR, self._model, self._staging[0], B)
        out = call()
        if self._owner is not None:   # every repeat starts from the same staging_in: a failed call wrote staging_out only
            out = fallback.encodec_ladder(self._owner, out, call, B, getattr(self._owner, "RANGE_OPTIONS", ()), self._DIR.pool_what,
                                          nonfinite_bit=self._DIR.nonfinite_bit)
        self.library_pushes += 1
        if not final:
            self._scatter(slots)
        return out

    # ---- device side --------------------------------------------------------------------------------------------------------------------------------
    def _device_call(self, x: torch.Tensor, final: bool, started: bool) -> torch.Tensor:
        """The bare library push, staging_in -> staging_out."""
        out, self._emb = self._DIR.call(self._model, self._staging[0], self._staging[1], x, final, self.n_q, self.keep_embeddings)
        return out

    def _device_copy(self, gather: bool, slots: List[int]) -> None:
        m = self._model
        host = torch.tensor(slots, dtype=torch.int32)
        dev = host.to(m.device)
        fn = (self._DIR.gather if gather else self._DIR.scatter)(m._h.lib)
        with torch.cuda.device(m.device):
            stream = _cabi.current_stream_handle(m.device)
            if gather:
                rc = fn(m._h.handle, self._pool.data_ptr(), self.slots, dev.data_ptr(), host.data_ptr(), len(slots), self._staging[0].data_ptr(), stream)
            else:
                rc = fn(m._h.handle, self._staging[1].data_ptr(), len(slots), dev.data_ptr(), host.data_ptr(), self._pool.data_ptr(), self.slots, stream)
        _cabi.check(rc, fn.__name__)

    def gather_scatter(self, slots: List[int], fresh: bool = False) -> None:
        """The two copies of a transaction without the push between them (tools/stream_pool_bench.py times them). ``fresh``: staging_out is first made
        the state of ``len(slots)`` new streams, for a pool whose last push was not of that many."""
        if fresh:
            _reset(self._DIR, self._model, self._staging[1], len(slots))
        self._gather(slots)
        self._scatter(slots)


class AcousticStreamPool(_StreamPool):
    """``sid = open()``; ``push({sid: samples [n], ...}) -> {sid: int16 [n_q, t]}`` on the device (``t`` may be 0); ``flush(sid | {sid, ...}) ->
    {sid: int16 [n_q, t_last]}`` frees the slots; ``close(sid)``; ``live``.

    Every stream is an :class:`AcousticStream` of its own as far as its tokens go — the tokens of one-shot ``encode`` of its audio — but the ids of one
    call that are in the same phase with the same number of whole frames go through ONE library push (see :class:`_StreamPool`). ``flush`` groups by
    (started, exact number of held samples); a stream that never started is the one-shot case and needs at least 321 samples, as the library says.

    ``push_fn(samples [B, n], final, started) -> codes [B, n_q, t]``; ``keep_embeddings``: ``last_embeddings = {sid: [t, 128]}`` of the last call.

    ``open(sample_rate=r)``: that stream takes raw samples at ``r`` Hz (float32 or int16, torch or numpy), resampled on the device at stream-global
    positions (resample_stream.py). All such streams of one ``push`` / ``flush`` call, whatever their rates, share ONE resample
    launch; what it gives enters the streams' ``held`` samples before any library push, so it outlives one that fails.
    """
    _DIR = _ENCODE

    def __init__(self, encoder=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None, n_q: Optional[int] = None, resampler=None):
        self.n_q = int(n_q if n_q is not None else encoder.n_q)
        self._resampler = resampler
        super().__init__(encoder, slots, push_fn, gather_fn, scatter_fn, owner)

    def open(self, sample_rate: Optional[int] = None) -> int:
        """A new stream in the lowest free slot; its id. ``sample_rate``: the rate of the raw samples it will be pushed (None: float at the model's rate)."""
        rate = None
        if sample_rate is not None:
            rate, self._resampler = _rate_state(self._model, sample_rate, 1, self._resampler)
        sid = super().open()
        self._rows[sid].rate = rate
        return sid


class AcousticDecodeStreamPool(_StreamPool):
    """``sid = open()``; ``push({sid: tokens [K, t], ...}) -> {sid: float32 [320 * t']}`` on the device; ``flush(sid | {sid, ...})``; ``close(sid)``; ``live``.

    Every stream behaves as an :class:`AcousticDecodeStream` of its own (tokens are held until 7 frames are there; ``flush`` decodes what a stream that
    never started still holds, and with fewer than 7 frames raises what one-shot decode raises); the ids of one call with the same (started, K, frames)
    go through ONE library push (see :class:`_StreamPool`). ``push_fn(tokens [B, K, t], started) -> wav [B, 320 * t]``.
    """
    _DIR = _DECODE

    def __init__(self, decoder=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None):
        super().__init__(decoder, slots, push_fn, gather_fn, scatter_fn, owner)
