"""Streaming acoustic encode and decode: audio (tokens) pushed in pieces, the tokens (audio) of the whole
(``at_encodec_encode_stream_checked`` / ``at_encodec_decode_stream_checked``).

``AcousticEncoder.new_stream(batch)`` returns an :class:`AcousticStream`. After any sequence of ``push`` calls and one ``flush`` the
concatenated tokens are the tokens one-shot ``encode`` gives for the concatenated audio, in memory bounded by the largest push.
The stream holds the device state of the library (two buffers, swapped when a push succeeded) and, on the host side, the samples that
do not fill a frame yet.

``AcousticDecoder.new_stream(batch)`` returns an :class:`AcousticDecodeStream`, the way back: tokens pushed frame by frame, the waveform one-shot
``decode`` gives for the concatenated tokens, 320 samples per frame as they arrive.

``new_stream_pool(slots)`` of either returns a pool (:class:`AcousticStreamPool`, :class:`AcousticDecodeStreamPool`): streams that start and finish on
their own, batched per call by phase and length.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Iterable, List, Optional, Union

import torch

from . import _cabi, fallback
from . import weights as W

HOP = W.ENCODEC_HOP          # 320 samples per frame
FIRST_PUSH_FRAMES = 7        # the library's minimum for the first push of a stream (include/audiotoken_hip.h)
SAMPLE_RATE = 24_000         # EnCodec's rate: what a stream without an encoder (push_fn) resamples to


class AcousticStream:
    """``push(samples [B, n]) -> int16 [B, n_q, t]`` on the device (``t`` may be 0), ``flush() -> int16 [B, n_q, t_last]``, ``reset()``.

    All ``batch`` rows advance in lockstep. A push is a transaction: the library reads one state buffer and writes the other; when the
    device status word of the push is non-zero the push is repeated from the untouched input state on the safe kernels, by the ladder
    ``AcousticEncoder.verified`` repeats a batch with (audiotoken_amd/fallback.py; bit 1: this push on the bf16x3 kernels, counted in ``fallback_batches``, the next push on
    f16x2 again; bit 0: the LSTM route is switched for the rest of the handle's life). Reading the status word synchronises once per push.

    ``push_fn(samples [B, n], final) -> codes [B, n_q, t]`` replaces the device call (the host-side buffering is tested with a stub).

    ``sample_rate``: the stream takes RAW samples at that rate (float32 or int16, torch or numpy) and resamples them on the device at stream-global
    positions, carrying the source tail across pushes (resample_stream.py): the tokens are those of the whole signal resampled
    once. The resampled samples enter the residual buffering below like pushed ones. None: samples are float at the model's rate, as ever.
    """

    def __init__(self, encoder=None, batch: int = 1, push_fn: Optional[Callable] = None, n_q: Optional[int] = None, sample_rate: Optional[int] = None,
                 resampler=None):
        assert batch >= 1, "batch must be >= 1"
        self._enc = encoder
        self.batch = int(batch)
        self._rate = None
        if sample_rate is not None:
            from . import resample_stream as RS
            model_rate = encoder.config.model_sample_rate if encoder is not None else SAMPLE_RATE
            self._rate = RS.RateState(sample_rate, model_rate, self.batch)
            self._resampler = resampler if resampler is not None else (encoder.resampler() if encoder is not None else RS.HostResampler(model_rate))
        self.n_q = int(n_q if n_q is not None else encoder.n_q)
        self._push_fn = push_fn if push_fn is not None else self._device_push
        self._state = None
        self.keep_embeddings = False   # parity tap: when set, every library push also leaves its pre-quantiser embedding [B, t, 128] in last_embeddings
        self.last_embeddings: Optional[torch.Tensor] = None
        if push_fn is None:
            lib = encoder._h.lib
            nbytes = lib.at_encodec_stream_state_bytes(encoder._h.handle, self.batch)
            self._state = [torch.empty(nbytes, dtype=torch.uint8, device=encoder.device) for _ in range(2)]
        self.reset()

    # ---- host side: residual buffering ------------------------------------------------------------------------------------------
    def reset(self) -> None:
        """Forget everything: the next push starts a new stream (h = c = 0, true left reflect padding)."""
        self._held: Optional[torch.Tensor] = None   # [B, < 320 (or < the first push's minimum)] samples not yet consumed
        self._started = False
        self._finished = False
        self.frames_emitted = 0
        if self._rate is not None:
            self._rate.reset()
        if self._state is not None:
            enc = self._enc
            with torch.cuda.device(enc.device):
                rc = enc._h.lib.at_encodec_stream_reset(enc._h.handle, self._state[0].data_ptr(), self.batch, _cabi.current_stream_handle(enc.device))
            _cabi.check(rc, "at_encodec_stream_reset")

    @property
    def fallback_batches(self) -> int:
        return self._enc.fallback_batches if self._enc is not None else 0

    def _empty(self, like: torch.Tensor) -> torch.Tensor:
        dev = self._enc.device if self._enc is not None else like.device
        return torch.empty((self.batch, self.n_q, 0), dtype=torch.int16, device=dev)

    def _check(self, samples: torch.Tensor) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("AcousticStream: push after flush(); call reset() to start a new stream")
        assert samples.dim() == 2 and samples.shape[0] == self.batch, f"samples must be [{self.batch}, n]"
        if self._enc is not None:
            samples = samples.to(device=self._enc.device, dtype=torch.float32)
        return samples

    def _resampled(self, samples, final: bool) -> torch.Tensor:
        """Raw samples at the stream's rate (None: none, the flush) -> what they add to the signal at the model's rate, float32 [B, m]. The source tail
        moves on here; the result goes into ``_held`` at once, so it outlives a push of the library that fails."""
        rs = self._rate
        window, n_new = rs.window(samples, self._enc.device if self._enc is not None else None)
        from .resample_stream import plan_push
        plan = plan_push(rs.pos, n_new, final)
        out = torch.stack(self._resampler.run(rs.jobs(window, plan))) if plan.out_len else window.new_zeros((self.batch, 0), dtype=torch.float32)
        rs.advance(window, plan)
        self._held = out if self._held is None else torch.cat([self._held, out], dim=1)
        return out[:, :0]

    def push(self, samples: torch.Tensor) -> torch.Tensor:
        if self._rate is not None:
            if self._finished:
                raise RuntimeError("AcousticStream: push after flush(); call reset() to start a new stream")
            samples = self._resampled(samples, False)
        samples = self._check(samples)
        held = samples if self._held is None else torch.cat([self._held, samples], dim=1)
        n = held.shape[1] // HOP * HOP
        if n == 0 or (not self._started and n < FIRST_PUSH_FRAMES * HOP):
            self._held = held
            self.last_embeddings = None
            return self._empty(samples)
        codes = self._push_fn(held[:, :n].contiguous(), False)
        self._held = held[:, n:]
        self._started = True
        self.frames_emitted += codes.shape[-1]
        return codes

    def flush(self) -> torch.Tensor:
        """The last frame(s): what is held goes out with the one-shot path's right-edge padding. The stream is finished afterwards."""
        if self._finished:
            raise RuntimeError("AcousticStream: flush() twice; call reset() to start a new stream")
        if self._rate is not None:
            self._resampled(None, True)
        held = self._held
        self._held = None
        self._finished = True
        if held is None or held.shape[1] == 0:
            self.last_embeddings = None
            return self._empty(held if held is not None else torch.empty(0))
        codes = self._push_fn(held.contiguous(), True)
        self.frames_emitted += codes.shape[-1]
        return codes

    # ---- device side: one transaction -------------------------------------------------------------------------------------------
    def _call(self, x: torch.Tensor, final: bool) -> torch.Tensor:
        enc = self._enc
        lib = enc._h.lib
        B, n = x.shape
        T = -(-n // HOP)
        codes = torch.empty((B, self.n_q, T), dtype=torch.int16, device=enc.device)
        emb = torch.empty((B, T, W.ENCODEC_DIM), dtype=torch.float32, device=enc.device) if self.keep_embeddings else None
        self.last_embeddings = emb
        nbytes = lib.at_encodec_stream_workspace_bytes(enc._h.handle, B, n)
        ws = enc._workspace(nbytes)
        t_out = C.c_int(0)
        with torch.cuda.device(enc.device):
            rc = lib.at_encodec_encode_stream_checked(enc._h.handle, self._state[0].data_ptr(), self._state[1].data_ptr(), x.data_ptr(), B, n,
                                                      1 if final else 0, self.n_q, codes.data_ptr(), C.byref(t_out), _cabi.ptr(emb), ws.data_ptr(), nbytes,
                                                      _cabi.current_stream_handle(enc.device), enc._status.data_ptr())
        _cabi.check(rc, "at_encodec_encode_stream_checked")
        assert t_out.value == T, (t_out.value, T)
        return codes

    def _device_push(self, x: torch.Tensor, final: bool) -> torch.Tensor:
        enc = self._enc
        # every repeat starts from the same input state: a failed call wrote the other buffer only
        codes = fallback.encodec_ladder(enc, self._call(x, final), lambda: self._call(x, final), self.batch, enc.RANGE_OPTIONS, "acoustic stream push")
        self._state.reverse()   # success: the written buffer is the next push's input
        return codes


class AcousticDecodeStream:
    """``push(tokens [B, K, t]) -> float32 [B, 320 * t']`` on the device, ``flush()``, ``reset()``.

    ``t'`` is ``t`` once the stream has started; before that, tokens are held until ``FIRST_PUSH_FRAMES`` frames are there (``t' = 0``) and then go
    out together: the first device push is a one-shot decode of its frames, whose left reflect padding needs 7 of them. ``flush()`` decodes what is
    still held, which only happens when the stream never started; with fewer than 7 frames in total it raises what one-shot decode raises for that
    ``T``. A started stream holds nothing, so its ``flush()`` returns ``[B, 0]``.

    A push is a transaction, as in :class:`AcousticStream`: the library reads one state buffer and writes the other, the status word is read once per
    push (one synchronisation), a non-zero status repeats the push from the untouched input state by ``fallback.encodec_ladder`` with
    ``AcousticDecoder.RANGE_OPTIONS``, and the two buffers are swapped on success.

    ``push_fn(tokens [B, K, t]) -> wav [B, 320 * t]`` replaces the device call (the host-side buffering is tested with a stub).
    """

    def __init__(self, decoder=None, batch: int = 1, push_fn: Optional[Callable] = None):
        assert batch >= 1, "batch must be >= 1"
        self._dec = decoder
        self.batch = int(batch)
        self._push_fn = push_fn if push_fn is not None else self._device_push
        self._state = None
        if push_fn is None:
            lib = decoder._h.lib
            nbytes = lib.at_encodec_decode_stream_state_bytes(decoder._h.handle, self.batch)
            self._state = [torch.empty(nbytes, dtype=torch.uint8, device=decoder.device) for _ in range(2)]
        self.reset()

    def reset(self) -> None:
        """Forget everything: the next push starts a new stream (h = c = 0, true left reflect padding)."""
        self._held: Optional[torch.Tensor] = None   # [B, K, < 7] frames of a stream that has not started
        self._started = False
        self._finished = False
        self.frames_emitted = 0
        if self._state is not None:
            dec = self._dec
            with torch.cuda.device(dec.device):
                rc = dec._h.lib.at_encodec_decode_stream_reset(dec._h.handle, self._state[0].data_ptr(), self.batch, _cabi.current_stream_handle(dec.device))
            _cabi.check(rc, "at_encodec_decode_stream_reset")

    @property
    def fallback_batches(self) -> int:
        return self._dec.fallback_batches if self._dec is not None else 0

    def _empty(self, like: torch.Tensor) -> torch.Tensor:
        dev = self._dec.device if self._dec is not None else like.device
        return torch.empty((self.batch, 0), dtype=torch.float32, device=dev)

    def _emit(self, tokens: torch.Tensor) -> torch.Tensor:
        wav = self._push_fn(tokens.contiguous())
        self._started = True
        self.frames_emitted += tokens.shape[-1]
        return wav

    def push(self, tokens: torch.Tensor) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("AcousticDecodeStream: push after flush(); call reset() to start a new stream")
        assert tokens.dim() == 3 and tokens.shape[0] == self.batch, f"tokens must be [{self.batch}, K, t]"
        if self._dec is not None:
            tokens = tokens.to(device=self._dec.device, dtype=torch.long)
        if self._started:
            return self._emit(tokens) if tokens.shape[-1] > 0 else self._empty(tokens)
        held = tokens if self._held is None else torch.cat([self._held, tokens], dim=-1)
        if held.shape[-1] < FIRST_PUSH_FRAMES:
            self._held = held
            return self._empty(tokens)
        self._held = None
        return self._emit(held)

    def flush(self) -> torch.Tensor:
        """What is still held (a stream that never reached 7 frames); the stream is finished afterwards."""
        if self._finished:
            raise RuntimeError("AcousticDecodeStream: flush() twice; call reset() to start a new stream")
        held = self._held
        self._held = None
        self._finished = True
        if held is None or held.shape[-1] == 0:
            return self._empty(held if held is not None else torch.empty(0))
        return self._emit(held)   # fewer than 7 frames in total: the library refuses it as it refuses a one-shot decode of that T

    # ---- device side: one transaction -------------------------------------------------------------------------------------------
    def _call(self, codes: torch.Tensor) -> torch.Tensor:
        dec = self._dec
        lib = dec._h.lib
        B, K, t = codes.shape
        wav = torch.empty((B, HOP * t), dtype=torch.float32, device=dec.device)
        nbytes = lib.at_encodec_decode_stream_workspace_bytes(dec._h.handle, B, t)
        ws = dec._workspace(nbytes)
        with torch.cuda.device(dec.device):
            rc = lib.at_encodec_decode_stream_checked(dec._h.handle, self._state[0].data_ptr(), self._state[1].data_ptr(), codes.data_ptr(), B, K, t,
                                                      wav.data_ptr(), ws.data_ptr(), nbytes, _cabi.current_stream_handle(dec.device), dec._status.data_ptr())
        _cabi.check(rc, "at_encodec_decode_stream_checked")
        return wav

    def _device_push(self, codes: torch.Tensor) -> torch.Tensor:
        dec = self._dec
        # every repeat starts from the same input state: a failed call wrote the other buffer only
        wav = fallback.encodec_ladder(dec, self._call(codes), lambda: self._call(codes), self.batch, dec.RANGE_OPTIONS, "acoustic decode stream push",
                                      nonfinite_bit=False)
        self._state.reverse()   # success: the written buffer is the next push's input
        return wav


# ======================================================================================================================================================
# Stream pools: the rows of a push still advance in lockstep, but WHICH streams form the rows changes from call to call
# ======================================================================================================================================================
class _Row:
    """Host-side record of one open stream of a pool."""
    __slots__ = ("slot", "held", "started", "rate")

    def __init__(self, slot: int):
        self.slot = slot
        self.rate = None                           # encode: resample_stream.RateState of a stream opened with a sample rate of its own
        self.held: Optional[torch.Tensor] = None   # encode: samples [< 320 (or < the first push's minimum)]; decode: tokens [K, < 7]
        self.started = False


class _StreamPool:
    """What the two pools share: slots, ids, and the transaction of one group.

    The per-stream state lives in row ``slot`` of a pool state for ``slots`` streams. One GROUP — ids in the same phase pushing the same length — is one
    library push of ``B = len(group)`` on two staging states: ``gather`` (pool -> staging_in; a starting group resets staging_in instead), the unchanged
    lockstep push staging_in -> staging_out with its status word read once and ``fallback.encodec_ladder`` repeating it from staging_in when it is
    non-zero, and only then ``scatter`` (staging_out -> pool; not after a final push, whose slots are free). A failed push never reaches the pool.

    ``push_fn``, ``gather_fn(slots)`` and ``scatter_fn(slots)`` replace the three device calls (``push_fn`` is the BARE library push, which also gets
    ``started``); ``owner`` is then what the ladder reads the status from (None: no status, no repeats). The bookkeeping is tested on the CPU that way.
    """
    _WHAT = ""
    _NONFINITE = True
    _LIB = ""   # "at_encodec_stream" / "at_encodec_decode_stream": prefix of _state_bytes, _reset, _gather, _scatter

    def __init__(self, model=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None):
        assert slots >= 1, "slots must be >= 1"
        assert (push_fn is None) == (gather_fn is None) == (scatter_fn is None), "push_fn, gather_fn and scatter_fn replace the device calls together"
        self._model = model
        self.slots = int(slots)
        self._rows: Dict[int, _Row] = {}
        self._free: List[int] = list(range(self.slots))
        self._next_id = 0
        self.library_pushes = 0    # groups pushed: one library push each (repeats of a failed push not counted)
        self._push = push_fn if push_fn is not None else self._device_call
        self._gather = gather_fn if gather_fn is not None else (lambda slots: self._device_copy("gather", slots))
        self._scatter = scatter_fn if scatter_fn is not None else (lambda slots: self._device_copy("scatter", slots))
        self._owner = model if push_fn is None else owner
        self._pool = self._staging = None
        if push_fn is None:
            lib, h = model._h.lib, model._h.handle
            nbytes = getattr(lib, self._LIB + "_state_bytes")(h, self.slots)
            # the pool and two staging states, each large enough for every slot at once (a state of B streams is the first state_bytes(B) bytes)
            self._pool = torch.empty(nbytes, dtype=torch.uint8, device=model.device)
            self._staging = [torch.empty(nbytes, dtype=torch.uint8, device=model.device) for _ in range(2)]
            self._reset_state(self._pool, self.slots)

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

    @staticmethod
    def _ordered(groups: Dict) -> list:
        """The groups of one call in the order they are pushed: by ascending smallest id (ids ascending inside a group)."""
        return sorted(((key, sorted(ids)) for key, ids in groups.items()), key=lambda g: g[1][0])

    # ---- one group = one transaction ------------------------------------------------------------------------------------------------------------------
    def _transaction(self, slots: List[int], started: bool, final: bool, call: Callable):
        B = len(slots)
        if started:
            self._gather(slots)
        elif self._staging is not None:
            self._reset_state(self._staging[0], B)
        out = call()
        if self._owner is not None:   # every repeat starts from the same staging_in: a failed call wrote staging_out only
            out = fallback.encodec_ladder(self._owner, out, call, B, getattr(self._owner, "RANGE_OPTIONS", ()), self._WHAT, nonfinite_bit=self._NONFINITE)
        self.library_pushes += 1
        if not final:
            self._scatter(slots)
        return out

    # ---- device side --------------------------------------------------------------------------------------------------------------------------------
    def _reset_state(self, state: torch.Tensor, B: int) -> None:
        m = self._model
        with torch.cuda.device(m.device):
            rc = getattr(m._h.lib, self._LIB + "_reset")(m._h.handle, state.data_ptr(), B, _cabi.current_stream_handle(m.device))
        _cabi.check(rc, self._LIB + "_reset")

    def _device_copy(self, which: str, slots: List[int]) -> None:
        m = self._model
        host = torch.tensor(slots, dtype=torch.int32)
        dev = host.to(m.device)
        fn = getattr(m._h.lib, f"{self._LIB}_{which}")
        with torch.cuda.device(m.device):
            stream = _cabi.current_stream_handle(m.device)
            if which == "gather":
                rc = fn(m._h.handle, self._pool.data_ptr(), self.slots, dev.data_ptr(), host.data_ptr(), len(slots), self._staging[0].data_ptr(), stream)
            else:
                rc = fn(m._h.handle, self._staging[1].data_ptr(), len(slots), dev.data_ptr(), host.data_ptr(), self._pool.data_ptr(), self.slots, stream)
        _cabi.check(rc, f"{self._LIB}_{which}")


class AcousticStreamPool(_StreamPool):
    """``sid = open()``; ``push({sid: samples [n], ...}) -> {sid: int16 [n_q, t]}`` on the device (``t`` may be 0); ``flush(sid | {sid, ...}) ->
    {sid: int16 [n_q, t_last]}`` frees the slots; ``close(sid)``; ``live``.

    Every stream is an :class:`AcousticStream` of its own as far as its tokens go — the same residual buffering (what does not fill a frame is held, the
    first push waits for 7 frames), the tokens of one-shot ``encode`` of its audio — but the ids of one call that are in the same phase with the same
    number of whole frames go through ONE library push (see :class:`_StreamPool`). ``flush`` groups by (started, exact number of held samples); a stream
    that never started is the one-shot case and needs at least 321 samples, as the library says.

    ``push_fn(samples [B, n], final, started) -> codes [B, n_q, t]``; ``keep_embeddings``: ``last_embeddings = {sid: [t, 128]}`` of the last call.

    ``open(sample_rate=r)``: that stream takes raw samples at ``r`` Hz (float32 or int16, torch or numpy), resampled on the device at stream-global
    positions (resample_stream.py). All such streams of one ``push`` / ``flush`` call, whatever their rates, share ONE resample
    launch; what it gives enters the streams' ``held`` samples before any library push, so it outlives one that fails.
    """
    _WHAT = "acoustic stream pool push"
    _LIB = "at_encodec_stream"

    def __init__(self, encoder=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None, n_q: Optional[int] = None, resampler=None):
        self.n_q = int(n_q if n_q is not None else encoder.n_q)
        self._resampler = resampler
        self.keep_embeddings = False
        self.last_embeddings: Dict[int, torch.Tensor] = {}
        self._emb = None
        super().__init__(encoder, slots, push_fn, gather_fn, scatter_fn, owner)

    def _empty(self, like: torch.Tensor) -> torch.Tensor:
        dev = self._model.device if self._model is not None else like.device
        return torch.empty((self.n_q, 0), dtype=torch.int16, device=dev)

    def open(self, sample_rate: Optional[int] = None) -> int:
        """A new stream in the lowest free slot; its id. ``sample_rate``: the rate of the raw samples it will be pushed (None: float at the model's rate)."""
        rate = None
        if sample_rate is not None:
            from . import resample_stream as RS
            model_rate = self._model.config.model_sample_rate if self._model is not None else SAMPLE_RATE
            rate = RS.RateState(sample_rate, model_rate, 1)
            if self._resampler is None:
                self._resampler = self._model.resampler() if self._model is not None else RS.HostResampler(model_rate)
        sid = super().open()
        self._rows[sid].rate = rate
        return sid

    def _resample(self, rows: Dict[int, "_Row"], samples: Dict[int, Optional[torch.Tensor]], final: bool) -> Dict[int, torch.Tensor]:
        """The rows with a rate of their own: ONE launch turns their raw samples (None: none, the flush) into what they add at the model's rate, and
        their source tails move on. ``{sid: float32 [m]}``."""
        from .resample_stream import plan_push
        dev = self._model.device if self._model is not None else None
        todo, jobs = [], []
        for sid, row in rows.items():
            if row.rate is None:
                continue
            x = samples[sid]
            window, n_new = row.rate.window(None if x is None else _row_samples(x), dev)
            plan = plan_push(row.rate.pos, n_new, final)
            todo.append((sid, row, window, plan))
            jobs.extend(row.rate.jobs(window, plan))
        outs = self._resampler.run(jobs) if jobs else []
        res = {}
        for (sid, row, window, plan), y in zip(todo, outs):
            row.rate.advance(window, plan)
            res[sid] = y
        return res

    def _run(self, ids: List[int], xs: List[torch.Tensor], started: bool, final: bool, out: Dict[int, torch.Tensor]) -> None:
        x = torch.stack(xs).contiguous()
        codes = self._transaction([self._rows[i].slot for i in ids], started, final, lambda: self._push(x, final, started))
        for b, sid in enumerate(ids):
            out[sid] = codes[b]
            if self._emb is not None:
                self.last_embeddings[sid] = self._emb[b]
        self._emb = None

    def push(self, samples: Dict[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
        out: Dict[int, torch.Tensor] = {}
        self.last_embeddings = {}
        groups: Dict[tuple, List[int]] = {}
        held: Dict[int, torch.Tensor] = {}
        rows = {sid: self._row(sid, "push") for sid in sorted(samples)}
        if any(row.rate is not None for row in rows.values()):
            samples = dict(samples)
            for sid, y in self._resample(rows, samples, False).items():   # into `held` first: the source tail has moved on
                row = rows[sid]
                row.held = y if row.held is None else torch.cat([row.held, y])
                samples[sid] = y[:0]
        for sid in sorted(samples):
            row, x = self._row(sid, "push"), samples[sid]
            assert x.dim() == 1, "samples of a stream must be [n]"
            if self._model is not None:
                x = x.to(device=self._model.device, dtype=torch.float32)
            h = x if row.held is None else torch.cat([row.held, x])
            frames = h.shape[0] // HOP
            if frames == 0 or (not row.started and frames < FIRST_PUSH_FRAMES):
                row.held = h
                out[sid] = self._empty(x)
            else:
                held[sid] = h
                groups.setdefault((row.started, frames), []).append(sid)
        for (started, frames), ids in self._ordered(groups):
            n = frames * HOP
            self._run(ids, [held[i][:n] for i in ids], started, False, out)
            for i in ids:   # the group's push succeeded: its rows have moved on
                self._rows[i].held = held[i][n:]
                self._rows[i].started = True
        return out

    def flush(self, sids: Union[int, Iterable[int]]) -> Dict[int, torch.Tensor]:
        """The last frame(s) of these streams: what they hold goes out with the one-shot path's right-edge padding. Their slots are free afterwards."""
        sids = [sids] if isinstance(sids, int) else sorted(set(sids))
        out: Dict[int, torch.Tensor] = {}
        self.last_embeddings = {}
        groups: Dict[tuple, List[int]] = {}
        rows = {sid: self._row(sid, "flush") for sid in sids}
        if any(row.rate is not None for row in rows.values()):
            for sid, y in self._resample(rows, {sid: None for sid in rows}, True).items():
                row = rows[sid]
                row.held = y if row.held is None else torch.cat([row.held, y])
        for sid, row in rows.items():
            n = 0 if row.held is None else row.held.shape[0]
            if n == 0:
                out[sid] = self._empty(row.held if row.held is not None else torch.empty(0))
            else:
                groups.setdefault((row.started, n), []).append(sid)
        try:
            for (started, n), ids in self._ordered(groups):
                self._run(ids, [rows[i].held for i in ids], started, True, out)
        finally:   # finished, whatever the library said about a clip below its minimum
            for sid, row in rows.items():
                self._release(row, sid)
        return out

    def _device_call(self, x: torch.Tensor, final: bool, started: bool) -> torch.Tensor:
        enc = self._model
        lib = enc._h.lib
        B, n = x.shape
        T = -(-n // HOP)
        codes = torch.empty((B, self.n_q, T), dtype=torch.int16, device=enc.device)
        self._emb = torch.empty((B, T, W.ENCODEC_DIM), dtype=torch.float32, device=enc.device) if self.keep_embeddings else None
        nbytes = lib.at_encodec_stream_workspace_bytes(enc._h.handle, B, n)
        ws = enc._workspace(nbytes)
        t_out = C.c_int(0)
        with torch.cuda.device(enc.device):
            rc = lib.at_encodec_encode_stream_checked(enc._h.handle, self._staging[0].data_ptr(), self._staging[1].data_ptr(), x.data_ptr(), B, n,
                                                      1 if final else 0, self.n_q, codes.data_ptr(), C.byref(t_out), _cabi.ptr(self._emb), ws.data_ptr(), nbytes,
                                                      _cabi.current_stream_handle(enc.device), enc._status.data_ptr())
        _cabi.check(rc, "at_encodec_encode_stream_checked")
        assert t_out.value == T, (t_out.value, T)
        return codes


def _row_samples(x):
    """Raw samples [n] of one pool stream as the one-row batch [1, n] a RateState takes."""
    import numpy as np
    x = torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x
    assert x.dim() == 1, "samples of a stream must be [n]"
    return x[None]


class AcousticDecodeStreamPool(_StreamPool):
    """``sid = open()``; ``push({sid: tokens [K, t], ...}) -> {sid: float32 [320 * t']}`` on the device; ``flush(sid | {sid, ...})``; ``close(sid)``; ``live``.

    Every stream behaves as an :class:`AcousticDecodeStream` of its own (tokens are held until 7 frames are there; ``flush`` decodes what a stream that
    never started still holds, and with fewer than 7 frames raises what one-shot decode raises); the ids of one call with the same (started, K, frames)
    go through ONE library push (see :class:`_StreamPool`). ``push_fn(tokens [B, K, t], started) -> wav [B, 320 * t]``.
    """
    _WHAT = "acoustic decode stream pool push"
    _NONFINITE = False
    _LIB = "at_encodec_decode_stream"

    def __init__(self, decoder=None, slots: int = 1, push_fn: Optional[Callable] = None, gather_fn: Optional[Callable] = None,
                 scatter_fn: Optional[Callable] = None, owner=None):
        super().__init__(decoder, slots, push_fn, gather_fn, scatter_fn, owner)

    def _empty(self, like: torch.Tensor) -> torch.Tensor:
        dev = self._model.device if self._model is not None else like.device
        return torch.empty((0,), dtype=torch.float32, device=dev)

    def _run_groups(self, groups: Dict[tuple, List[int]], toks: Dict[int, torch.Tensor], out: Dict[int, torch.Tensor]) -> None:
        for (started, K, t), ids in self._ordered(groups):
            x = torch.stack([toks[i] for i in ids]).contiguous()
            wav = self._transaction([self._rows[i].slot for i in ids], started, False, lambda: self._push(x, started))
            for b, sid in enumerate(ids):
                out[sid] = wav[b]
                self._rows[sid].held = None
                self._rows[sid].started = True

    def push(self, tokens: Dict[int, torch.Tensor]) -> Dict[int, torch.Tensor]:
        out: Dict[int, torch.Tensor] = {}
        groups: Dict[tuple, List[int]] = {}
        toks: Dict[int, torch.Tensor] = {}
        for sid in sorted(tokens):
            row, x = self._row(sid, "push"), tokens[sid]
            assert x.dim() == 2, "tokens of a stream must be [K, t]"
            if self._model is not None:
                x = x.to(device=self._model.device, dtype=torch.long)
            if not row.started:
                x = x if row.held is None else torch.cat([row.held, x], dim=-1)
                if x.shape[-1] < FIRST_PUSH_FRAMES:
                    row.held = x
                    out[sid] = self._empty(x)
                    continue
            if x.shape[-1] == 0:
                out[sid] = self._empty(x)
                continue
            toks[sid] = x
            groups.setdefault((row.started, x.shape[0], x.shape[-1]), []).append(sid)
        self._run_groups(groups, toks, out)
        return out

    def flush(self, sids: Union[int, Iterable[int]]) -> Dict[int, torch.Tensor]:
        """What these streams still hold (streams that never reached 7 frames); their slots are free afterwards."""
        sids = [sids] if isinstance(sids, int) else sorted(set(sids))
        out: Dict[int, torch.Tensor] = {}
        groups: Dict[tuple, List[int]] = {}
        toks: Dict[int, torch.Tensor] = {}
        rows = {sid: self._row(sid, "flush") for sid in sids}
        for sid, row in rows.items():
            if row.held is None or row.held.shape[-1] == 0:
                out[sid] = self._empty(row.held if row.held is not None else torch.empty(0))
            else:   # fewer than 7 frames in total: the library refuses it as it refuses a one-shot decode of that T
                toks[sid] = row.held
                groups.setdefault((False, row.held.shape[0], row.held.shape[-1]), []).append(sid)
        try:
            self._run_groups(groups, toks, out)
        finally:
            for sid, row in rows.items():
                self._release(row, sid)
        return out

    def _device_call(self, codes: torch.Tensor, started: bool) -> torch.Tensor:
        dec = self._model
        lib = dec._h.lib
        B, K, t = codes.shape
        wav = torch.empty((B, HOP * t), dtype=torch.float32, device=dec.device)
        nbytes = lib.at_encodec_decode_stream_workspace_bytes(dec._h.handle, B, t)
        ws = dec._workspace(nbytes)
        with torch.cuda.device(dec.device):
            rc = lib.at_encodec_decode_stream_checked(dec._h.handle, self._staging[0].data_ptr(), self._staging[1].data_ptr(), codes.data_ptr(), B, K, t,
                                                      wav.data_ptr(), ws.data_ptr(), nbytes, _cabi.current_stream_handle(dec.device), dec._status.data_ptr())
        _cabi.check(rc, "at_encodec_decode_stream_checked")
        return wav
