"""Streaming acoustic encode and decode: audio (tokens) pushed in pieces, the tokens (audio) of the whole
(``at_encodec_encode_stream_checked`` / ``at_encodec_decode_stream_checked``).

``AcousticEncoder.new_stream(batch)`` returns an :class:`AcousticStream`. After any sequence of ``push`` calls and one ``flush`` the
concatenated tokens are the tokens one-shot ``encode`` gives for the concatenated audio, in memory bounded by the largest push.
The stream holds the device state of the library (two buffers, swapped when a push succeeded) and, on the host side, the samples that
do not fill a frame yet.

``AcousticDecoder.new_stream(batch)`` returns an :class:`AcousticDecodeStream`, the way back: tokens pushed frame by frame, the waveform one-shot
``decode`` gives for the concatenated tokens, 320 samples per frame as they arrive.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Optional

import torch

from . import _cabi, fallback
from . import weights as W

HOP = W.ENCODEC_HOP          # 320 samples per frame
FIRST_PUSH_FRAMES = 7        # the library's minimum for the first push of a stream (include/audiotoken_hip.h)


class AcousticStream:
    """``push(samples [B, n]) -> int16 [B, n_q, t]`` on the device (``t`` may be 0), ``flush() -> int16 [B, n_q, t_last]``, ``reset()``.

    All ``batch`` rows advance in lockstep. A push is a transaction: the library reads one state buffer and writes the other; when the
    device status word of the push is non-zero the push is repeated from the untouched input state on the safe kernels, by the ladder
    ``AcousticEncoder.verified`` repeats a batch with (audiotoken_amd/fallback.py; bit 1: this push on the bf16x3 kernels, counted in ``fallback_batches``, the next push on
    f16x2 again; bit 0: the LSTM route is switched for the rest of the handle's life). Reading the status word synchronises once per push.

    ``push_fn(samples [B, n], final) -> codes [B, n_q, t]`` replaces the device call (the host-side buffering is tested with a stub).
    """

    def __init__(self, encoder=None, batch: int = 1, push_fn: Optional[Callable] = None, n_q: Optional[int] = None):
        assert batch >= 1, "batch must be >= 1"
        self._enc = encoder
        self.batch = int(batch)
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

    def push(self, samples: torch.Tensor) -> torch.Tensor:
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
