"""Semantic ids -> audio as a stream: ``push`` ids as they arrive, get audio as it turns final. The three stages are the offline ones
(``to_acoustic(long_form=True)``, ``to_fine``, ``AcousticDecodeStream``); only WHEN a window runs changes, so the coarse ids and the fine codes are those of
the offline calls on the whole source, id for id. ``stream_schedule`` is the rule as a pure-Python twin; ``gpt_stream_rounds`` / ``fine_stream_rounds`` are
the twins of the library's host schedulers (csrc/gpt.h ``GptStreamSchedule``, csrc/fine.h ``FineStreamSchedule``).

The latency has a floor: the fine model is non-causal over ``W`` frames, so the first audio of a long source needs ``W`` coarse frames (at ``W = 1024``,
``r = 3``: 2048 GPT ids, 683 source ids); after that audio arrives every ``W / 2`` frames. A source shorter than ``W`` frames gets all its audio at ``flush()``."""
from __future__ import annotations

import ctypes as C
from typing import List, Optional

import numpy as np
import torch

from . import _cabi
from .fine_decoder import N_PASSES
from .semantic_decoder import FINISH, MAX_SOURCE_IDS, check_truncation, check_windows, default_window

HOP_SAMPLES = 320   # audio samples per frame


# ---- the rule ----------------------------------------------------------------------------------------------------------------------------------------
def gpt_windows_run(n_in: int, S: int, H: int) -> int:
    """Non-final GPT windows that have run once ``n_in`` ids were pushed: window k runs as soon as ``n_in > k H + S`` (one id past it must exist)."""
    return (n_in - S - 1) // H + 1 if n_in > S else 0


def fine_windows_run(T: int, W: int) -> int:
    """Fine windows that have run once ``T`` coarse frames exist: window j runs at ``start = j H`` as soon as ``j H + W <= T``."""
    return (T - W) // (W // 2) + 1 if T >= W else 0


def fine_capacity(W: int) -> int:
    """Cells of the stream's window onto the fine row: from the start of the last window run (at most ``W + H`` frames wait there for the next one) plus
    room to take frames in; a GPT window that adds more is handed over in rounds."""
    return 2 * W


def gpt_window_ids(k: int, S: int, H: int, r: int):
    """``(stream position of its first new id, new ids)`` of NON-final window k."""
    carry = r * (S - H) if k else 0
    return r * k * H + carry, r * S - carry


def gpt_stream_rounds(n_before: int, n_new: int, final: bool, S: int, H: int):
    """Twin of ``GptStreamSchedule``: the rounds of one push, ``(take, held, k_first, n_win, final_window, final_ids)``."""
    n, left, k, out, done = n_before, n_new, gpt_windows_run(n_before, S, H), [], False
    while not done:
        held = n - k * H
        take = min(left, 2 * S - held)
        n, left = n + take, left - take
        k_first, k = k, gpt_windows_run(n + 0, S, H)
        fw, fids = False, 0
        if left == 0:
            done = True
            if final:
                fw, fids = True, n - k * H
        if take > 0 or k > k_first or fw:
            out.append((take, held, k_first, k - k_first, int(fw), fids))
    return out


def fine_stream_rounds(T_before: int, n_new: int, final: bool, W: int):
    """Twin of ``FineStreamSchedule``: the rounds of one push, ``(take, first, held, j_first, n_win, pad, last_window, last_rel, emit_from, emit_to, shift)``."""
    H = W // 2
    first_of = lambda j: (j - 1) * H if j > 0 else 0
    T, left, j, out, done = T_before, n_new, fine_windows_run(T_before, W), [], False
    while not done:
        first = first_of(j)
        held = T - first
        take = min(left, fine_capacity(W) - held)
        T, left = T + take, left - take
        j_first, j = j, fine_windows_run(T, W)
        n_win, pad, last, rel, e0, e1 = j - j_first, 0, False, 0, j_first * H, j * H
        if left == 0:
            done = True
            if final:
                if T < W:
                    pad, n_win = W - T, 1
                elif (T - W) % H:
                    last, rel = True, j * H - (T - W)
                e1 = T
        shift = 0 if done and final else first_of(j) - first
        if take > 0 or n_win > 0 or last or e1 > e0:
            out.append((take, first, held, j_first, n_win, pad, int(last), rel, e0, e1, shift))
    return out


def stream_schedule(pushes, S: int, H_g: int, r: int, block: int, W: int, final_budget_result: Optional[int] = None, max_new_tokens: int = 1024):
    """The stream's rule for one source pushed as ``pushes`` (ids per push) and then flushed: one event per call, the flush last. An event is a dict:
    ``gpt`` the GPT windows run ``[(k, final)]``, ``new_ids`` the stream ids they produced, ``fine`` the fine windows run ``[(start, fill)]`` (the
    offline ``fine_windows`` form), ``emit`` the frames ``(from, to)`` that turned final and go to the decode stream as one piece, ``held`` the most
    frames the window onto the fine row held. ``final_budget_result``: the ids the final window produced (the device decides; default: its budget)."""
    check_windows(S, H_g, r, block)
    H = W // 2
    events, n_in, T, stream_len = [], 0, 0, 0
    for i, n_new in enumerate(list(pushes) + [0]):
        final = i == len(pushes)
        if final and n_in == 0:
            raise ValueError("flush() with nothing pushed")
        gpt, new_ids = [], 0
        for take, held, k_first, n_win, fw, fids in gpt_stream_rounds(n_in, n_new, final, S, H_g):
            for k in range(k_first, k_first + n_win):
                gpt.append((k, False))
                new_ids += gpt_window_ids(k, S, H_g, r)[1]
            if fw:
                k = k_first + n_win
                carry = r * (S - H_g) if k else 0
                budget = min(max_new_tokens, block - (fids + 1 + carry))
                gpt.append((k, True))
                new_ids += budget if final_budget_result is None else int(final_budget_result)
        n_in += n_new
        stream_len += new_ids
        T_new = stream_len // 2          # coarse frame t exists once stream positions 2 t and 2 t + 1 do; a trailing unpaired id is dropped
        fine, held_max, e_from, e_to = [], 0, None, None
        if not (final and T_new == 0):
            for take, first, held, j_first, n_win, pad, last, rel, e0, e1, shift in fine_stream_rounds(T, T_new - T, final, W):
                held_max = max(held_max, held + take + pad)
                for j in range(j_first, j_first + n_win):
                    fine.append((j * H, j * H))
                if last:
                    fine.append((T_new - W, T_new - W + rel))
                if e1 > e0:
                    e_from, e_to = (e0 if e_from is None else e_from), e1
        T = T_new
        events.append({"gpt": gpt, "new_ids": new_ids, "fine": fine, "emit": (e_from, e_to) if e_from is not None else None, "held": held_max, "n_in": n_in, "frames": T})
    return events


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------------
class _Draws:
    """A lazily drawn prefix of ``Philox(seed).random(...)`` (float32): the stream never needs the source's length. Chunked ``.random`` calls on one
    generator continue the same sequence (tests/test_semantic_stream_cpu.py pins this)."""

    def __init__(self, seed: int, row: int, explicit=None, what: str = "uniforms"):
        self.row, self.what = int(row), what
        self.explicit = None if explicit is None else np.ascontiguousarray(explicit, dtype=np.float32).reshape(-1, self.row)
        self.gen = np.random.Generator(np.random.Philox(seed))
        self.have = np.zeros((0, self.row), dtype=np.float32)

    def rows(self, lo: int, hi: int) -> np.ndarray:
        if self.explicit is not None:
            if hi > self.explicit.shape[0]:
                raise ValueError(f"{self.what}: the stream needs entry {hi - 1}, the given array has {self.explicit.shape[0]}")
            return self.explicit[lo:hi]
        if hi > self.have.shape[0]:
            self.have = np.concatenate([self.have, self.gen.random((hi - self.have.shape[0], self.row), dtype=np.float32)])
        return self.have[lo:hi]


class SemanticAudioStream:
    """``push(ids) -> float32 (1, 320 * n)`` on the CPU (``n`` may be 0), ``flush()``, ``reset()``: one source of semantic ids to audio.

    ``gpt`` / ``fine`` / ``decoder``: a ``SemanticToAcoustic``, a ``CoarseToFine`` and an ``AcousticDecoder`` at 8 code books on one device. The coarse
    ids are those of ``gpt.to_acoustic_long(source, window, hop, max_new_tokens, temperature, top_k, uniforms=, top_p=, min_p=)`` and the fine codes those
    of ``fine.generate(codes, fine_temperature, uniforms=)`` on the whole source, with the same draws: stream position p of stage 1 draws ``uniforms[p]``,
    fine window j draws ``fine_uniforms[j]`` (``[n, 6, W]``); from ``seed`` both are the prefixes of what the offline call draws for one source. Explicit
    arrays are for tests; running past them raises before anything is launched. ``keep_codes``: keep what was produced (on the device) for
    ``coarse_ids`` / ``fine_codes``. Each object owns its device state, whose size does not depend on the source's length; several may be alive at once.
    Not built, and refused: ``voice=`` (the prompted schedule), and a second source without ``reset()``."""

    def __init__(self, gpt, fine, decoder, window: Optional[int] = None, hop: Optional[int] = None, max_new_tokens: int = 1024, temperature: float = 0.8,
                 top_k: int = 100, fine_temperature: Optional[float] = 0.5, seed: int = 0, uniforms=None, fine_uniforms=None, top_p: Optional[float] = None,
                 min_p: Optional[float] = None, keep_codes: bool = False, voice=None):
        if voice is not None:
            raise ValueError("audio_stream: voice= is not built for streams (the prompted schedule changes every window); use to_audio(long_form=True, voice=)")
        self._truncation = check_truncation(top_p, min_p)
        self.gpt, self.fine, self.decoder = gpt, fine, decoder
        cfg = gpt.config
        self.r, self.block, self.W = int(cfg.ids_per_source_token), gpt.block_size, fine.block_size
        self.S = default_window(cfg, self.block)[0] if window is None else int(window)
        self.H = (self.S // 2) // 2 * 2 if hop is None else int(hop)
        check_windows(self.S, self.H, self.r, self.block)
        self.max_new = int(max_new_tokens)
        if not 1 <= self.max_new <= 1024:
            raise ValueError(f"audio_stream: max_new_tokens must be 1 to 1024, got {self.max_new}")
        self.temperature, self.top_k, self.fine_temperature = float(temperature), int(top_k), fine_temperature
        self.seed, self.keep_codes = int(seed), bool(keep_codes)
        self._u_given, self._fu_given = uniforms, fine_uniforms
        if fine_uniforms is not None and np.shape(fine_uniforms)[1:] != (N_PASSES, self.W):
            raise ValueError(f"fine_uniforms must be float32 [n, {N_PASSES}, {self.W}] (window, code book, buffer position), got {np.shape(fine_uniforms)}")
        self.device = gpt.device
        with torch.cuda.device(self.device):
            n_g = int(gpt._fn("stream_state_bytes")(gpt.handle, self.S, self.H, self.r))
            n_f = int(fine._fn("stream_state_bytes")(fine.handle))
            if n_g == 0 or n_f == 0:
                raise _cabi.HipLibraryError(f"stream state size failed: {_cabi.last_error()}")
            self._gpt_state = torch.empty(n_g, dtype=torch.uint8, device=self.device)
            self._fine_state = torch.empty(n_f, dtype=torch.uint8, device=self.device)
            self._len = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._fin = torch.zeros(1, dtype=torch.int32, device=self.device)
            self._status = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._decode = decoder.new_stream(1)
        self.reset()

    @property
    def state_bytes(self):
        """``(GPT state, fine state)`` in bytes: fixed by the geometry and the models, whatever the source's length."""
        return self._gpt_state.numel(), self._fine_state.numel()

    def reset(self) -> None:
        """Forget the source: the next push starts a new one. The draws start over."""
        self._gpos, self._fpos = (C.c_int64 * 2)(0, 0), (C.c_int64 * 2)(0, 0)
        self._u = _Draws(self.seed, 1, self._u_given, "uniforms")
        self._fu = _Draws(self.seed, N_PASSES * self.W, self._fu_given, "fine_uniforms")
        self._windows: List[tuple] = []
        self._fine_run: List[tuple] = []
        self._ids: List[torch.Tensor] = []
        self._codes: List[torch.Tensor] = []
        self._finish: Optional[str] = None
        self._finished = False
        self.frames_out = 0
        self._status.zero_()
        self._decode.reset()

    ids_in = property(lambda self: int(self._gpos[0]))
    frames_in = property(lambda self: int(self._fpos[0]))

    @property
    def finish(self) -> Optional[str]:
        """After ``flush()``: "stop" | "max_new_tokens" | "block_size", as ``AcousticGeneration.finish``."""
        return self._finish

    @property
    def windows(self) -> List[tuple]:
        """The GPT windows that ran, ``(source_start, source_len, carry, new_ids)`` as ``AcousticGeneration.windows`` lists them."""
        return list(self._windows)

    @property
    def fine_windows_run(self) -> List[tuple]:
        """The fine windows that ran, ``(start, fill)`` as ``fine_decoder.fine_windows`` lists them."""
        return list(self._fine_run)

    @property
    def coarse_ids(self) -> torch.Tensor:
        """``keep_codes``: the stream's ids so far minus the acoustic offset, int64 on the CPU (``AcousticGeneration.ids`` of the offline call)."""
        self._kept()
        ids = torch.cat(self._ids) if self._ids else torch.empty(0, dtype=torch.int32)
        return ids.cpu().to(torch.int64) - self.gpt.config.ACOUSTIC_OFFSET

    @property
    def fine_codes(self) -> torch.Tensor:
        """``keep_codes``: the frames that turned final so far, int64 ``[8, n]`` on the CPU."""
        self._kept()
        return torch.cat(self._codes, dim=1).cpu() if self._codes else torch.empty((8, 0), dtype=torch.int64)

    def _kept(self) -> None:
        if not self.keep_codes:
            raise ValueError("audio_stream: coarse_ids / fine_codes need keep_codes=True")

    # ---- the two calls -----------------------------------------------------------------------------------------------------------------------------
    def push(self, ids) -> torch.Tensor:
        if self._finished:
            raise RuntimeError("SemanticAudioStream: push after flush(); call reset() to start a new source")
        cfg = self.gpt.config
        t = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)).reshape(-1)
        if t.numel() and (t.is_floating_point() or t.dtype == torch.bool):
            raise ValueError(f"audio_stream: ids must be integers, got {t.dtype}")
        t = t.to(torch.int64)
        if t.numel() and (int(t.min()) < 0 or int(t.max()) >= cfg.SEMANTIC_VOCAB_SIZE):
            raise ValueError(f"audio_stream: semantic ids must lie in [0, {cfg.SEMANTIC_VOCAB_SIZE})")
        if self.ids_in + t.numel() > MAX_SOURCE_IDS:
            raise ValueError(f"audio_stream: a source has at most {MAX_SOURCE_IDS} ids")
        return self._advance(t.to(torch.int32), False)

    def flush(self) -> torch.Tensor:
        """The final GPT window, the last fine window and the rest of the audio. The stream is finished afterwards."""
        if self._finished:
            raise RuntimeError("SemanticAudioStream: flush() twice; call reset() to start a new source")
        if self.ids_in == 0:
            raise RuntimeError("SemanticAudioStream: flush() with nothing pushed")
        return self._advance(torch.empty(0, dtype=torch.int32), True)

    def _advance(self, ids: torch.Tensor, final: bool) -> torch.Tensor:
        cfg, S, H, r, W = self.gpt.config, self.S, self.H, self.r, self.W
        n_before, n_new = self.ids_in, int(ids.numel())
        k0 = gpt_windows_run(n_before, S, H)
        k1 = gpt_windows_run(n_before + n_new, S, H)
        carry0 = r * (S - H) if k0 else 0
        p_base = r * k0 * H if k0 else 0
        first_new = p_base + carry0                       # == the stream's length so far
        new_ids = sum(gpt_window_ids(k, S, H, r)[1] for k in range(k0, k1))
        budget = 0
        if final:
            carry = r * (S - H) if k1 else 0
            budget = min(self.max_new, self.block - (n_before + n_new - k1 * H + 1 + carry))
        cap_ids = new_ids + budget
        # ---- everything that can be refused is refused here, before anything is launched
        u = self._u.rows(first_new, first_new + cap_ids).reshape(-1) if cap_ids else np.zeros(1, dtype=np.float32)
        T_before = self.frames_in
        j0 = fine_windows_run(T_before, W)
        greedy = self.fine_temperature is None
        if not final:   # the fine stage's part of this push is known now; flush() learns its length from the device
            fu, j_lo, n_emit, fine_rounds = self._fine_plan(T_before, new_ids // 2, False, greedy)
        dev = self.device
        out = []
        with torch.cuda.device(dev):
            d_ids = ids.to(dev) if n_new else None
            d_u = torch.from_numpy(np.ascontiguousarray(u)).to(dev)
            d_out = torch.empty(max(carry0 + cap_ids, 2), dtype=torch.int32, device=dev)
            stream = _cabi.current_stream_handle(dev)
            ran = C.c_int32(0)
            with self.gpt._truncated(*self._truncation):
                _cabi.check(self.gpt._fn("stream_push")(self.gpt.handle, self._gpt_state.data_ptr(), self._gpt_state.numel(), self._gpos, _cabi.ptr(d_ids), n_new,
                                                        1 if final else 0, S, H, r, cfg.SEMANTIC_OFFSET, cfg.SEMANTIC_VOCAB_SIZE, cfg.INFER_TOKEN,
                                                        cfg.ACOUSTIC_OFFSET, cfg.codebook_size, cfg.STOP_TOKEN, self.max_new, self.temperature, self.top_k,
                                                        d_u.data_ptr(), first_new, max(cap_ids, 0), d_out.data_ptr(), carry0 + cap_ids, self._len.data_ptr(),
                                                        self._fin.data_ptr(), C.byref(ran), stream, self._status.data_ptr()), "at_gpt_stream_push")
            for k in range(k0, k1):
                self._windows.append((k * H, S, r * (S - H) if k else 0, gpt_window_ids(k, S, H, r)[1]))
            if final:
                self._finished = True
                total, fin = int(self._len.item()), int(self._fin.item())   # the final length: the flush's one look at the device besides the flag poll
                self._finish = FINISH[fin]
                made = total - first_new - new_ids
                self._windows.append((k1 * H, n_before + n_new - k1 * H, r * (S - H) if k1 else 0, made))
                new_ids += made
                if total // 2 < 1:
                    raise ValueError(f"to_audio: source 0 produced no whole frame of coarse codes (finish: {self._finish})")
                fu, j_lo, n_emit, fine_rounds = self._fine_plan(T_before, total // 2 - T_before, True, greedy)
            if self.keep_codes and new_ids:
                self._ids.append(d_out[carry0:carry0 + new_ids].clone())
            n_frames = (first_new + new_ids) // 2 - T_before
            if n_frames or final:
                d_fu = None if greedy or fu is None else torch.from_numpy(np.ascontiguousarray(fu)).to(dev)
                d_emit = torch.empty((8, max(n_emit, 1)), dtype=torch.int64, device=dev)
                got, wins = C.c_int32(0), C.c_int32(0)
                _cabi.check(self.fine._fn("stream_push")(self.fine.handle, self._fine_state.data_ptr(), self._fine_state.numel(), self._fpos,
                                                         d_out.data_ptr() + 4 * carry0, n_frames, 1 if final else 0, cfg.ACOUSTIC_OFFSET, cfg.codebook_size,
                                                         1.0 if greedy else float(self.fine_temperature), 1 if greedy else 0, _cabi.ptr(d_fu), j_lo,
                                                         0 if fu is None else fu.shape[0], d_emit.data_ptr(), max(n_emit, 1), C.byref(got), C.byref(wins),
                                                         stream, self._status[1:].data_ptr()), "at_fine_stream_push")
                assert got.value == n_emit, (got.value, n_emit)
                self._fine_run.extend(fine_rounds)
                if n_emit:
                    piece = d_emit[:, :n_emit].contiguous() if n_emit != d_emit.shape[1] else d_emit
                    if self.keep_codes:
                        self._codes.append(piece.clone())
                    out.append(self._decode.push(piece.unsqueeze(0)))
            if final:
                out.append(self._decode.flush())
                status = self._status.tolist()   # the device has been waited for already
                if status[0] & 1:
                    raise ValueError("audio_stream: a source id lies outside the semantic vocabulary")
                if status[1] & 4:
                    raise ValueError("audio_stream: a stream id lies outside its code book")
            audio = torch.cat(out, dim=-1).cpu() if out else torch.empty((1, 0), dtype=torch.float32)
        self.frames_out += audio.shape[-1] // HOP_SAMPLES
        return audio

    def _fine_plan(self, T_before: int, n_frames: int, final: bool, greedy: bool):
        """What the fine stage does with ``n_frames`` more frames: (its windows' draws ``[n, 6 W]`` or None, the first window, the frames that turn final,
        the windows as ``(start, fill)``). Raises where explicit draws run out."""
        W, H = self.W, self.W // 2
        wins, n_emit, j_lo, j_hi = [], 0, None, None
        T = T_before + n_frames
        for take, first, held, j_first, n_win, pad, last, rel, e0, e1, shift in fine_stream_rounds(T_before, n_frames, final, W):
            for j in range(j_first, j_first + n_win):
                wins.append((j * H, j * H))
            if last:
                wins.append((T - W, T - W + rel))
            n = n_win + last
            if n:
                j_lo, j_hi = (j_first if j_lo is None else j_lo), j_first + n
            n_emit += e1 - e0
        fu = None
        if wins and not greedy:
            fu = self._fu.rows(j_lo, j_hi)
        return fu, (j_lo or 0), n_emit, wins
