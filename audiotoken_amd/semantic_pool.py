"""Semantic-to-audio stream pools: live streams that start, push and finish on their own share the GPT's ticks. Every stream follows §25's
rule unchanged (the same windows, allow sets, carry, finish rules and draws as ``audio_stream(seed=s)``); only WHEN a window runs, and beside which others,
changes. ``pool_schedule`` is the rule of one call as a pure-Python twin of ``GptPoolSchedule`` (csrc/gpt.h) and ``fine_pool_passes`` that of
``FinePoolSchedule`` (csrc/fine.h); ``GptStreamPool`` is stage 1 on its own (``SemanticToAcoustic.stream_pool``): its push gives each stream's new coarse
ids on the device; ``SemanticAudioStreamPool`` (``AudioToken.audio_stream_pool``) is built on it and adds the fine stage's pool and one decode stream pool."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional

import numpy as np
import torch

from . import _cabi
from .semantic_decoder import (CHECK_EVERY, DEFAULT_TICK_WINDOWS, FINISH, GEMM_ABOVE, MAX_SLOTS, MAX_SOURCE_IDS, check_truncation, check_windows, default_window)
from .fine_decoder import N_PASSES
from .semantic_stream import HOP_SAMPLES, _Draws, fine_stream_rounds, gpt_stream_rounds, gpt_window_ids, gpt_windows_run

MAX_POOL_STREAMS = 1024   # live streams of one pool (csrc/gpt.h: GPT_MAX_POOL_STREAMS)


def pool_max_len(S: int, H: int, r: int, block: int, max_new: int) -> int:
    """Positions of a pool's cache row: a non-final window fills ``S + 1 + r S``, a final one its prompt and at most ``max_new`` more."""
    return max(S + 1 + r * S, min(block, S + 1 + r * (S - H) + max_new))


# ---- the rule of one call ------------------------------------------------------------------------------------------------------------------------------
def pool_schedule(streams, S: int, H: int, r: int, block: int, max_new: int, slots: int, tick_tokens: int, final_steps=None, detail: bool = False):
    """One call of a pool (``GptPoolSchedule`` in csrc/gpt.h is the same arithmetic). ``streams``: per stream of the call, in ascending
    stream id, ``(ids before the call, ids pushed, flushed)``. Each stream's work is §25's for its push (``gpt_stream_rounds``). A round is global: round g
    of the call is round g of every stream that still has one. In a round a stream's windows form a chain (its non-final windows, then the final one), and
    the chains are §20's sources: waiting streams take free cache rows in ascending stream id, every running row steps, windows are admitted in slot order
    while the tick's list stays within ``tick_tokens``, a row whose chain is complete is handed on, and the round ends when every chain is complete. The
    flags are polled every ``CHECK_EVERY`` ticks of the call while some row is in a final window; ``final_steps[i]``: the sampler launches stream i's final
    window took (its new ids, plus one for a sampled STOP; default: its budget). Returns ``(rounds, ticks, placement)``: per round and stream its
    ``gpt_stream_rounds`` tuple or None, per tick ``(step tokens, windows started, prefill tokens, route, round)``, per stream ``(the slot of its last
    chain, first tick, last tick)`` with -1 where it ran no window. ``detail``: a fourth list, per tick ``(steps [(slot, stream, window)],
    starts [(slot, stream, window, prompt tokens, final)], polled, slots whose window waits)``."""
    check_windows(S, H, r, block)
    n = len(streams)
    if not 1 <= slots <= MAX_SLOTS:
        raise ValueError(f"pool: 1 to {MAX_SLOTS} slots, got {slots}")
    if tick_tokens < slots + pool_max_len(S, H, r, block, max_new):
        raise ValueError(f"pool: tick_tokens ({tick_tokens}) must hold a step of every slot and one whole window")
    per = [gpt_stream_rounds(int(b), int(m), bool(f), S, H) for b, m, f in streams]
    n_rounds = max([len(p) for p in per] + [0])
    rounds, ticks, events = [], [], []
    placement = [[-1, -1, -1] for _ in range(n)]
    for g in range(n_rounds):
        rd = [p[g] if g < len(p) else None for p in per]
        rounds.append(rd)
        chains = []
        for i, x in enumerate(rd):
            chain = []
            if x is not None:
                take, held, k_first, n_win, fw, fids = x
                for k in range(k_first, k_first + n_win):
                    carry = r * (S - H) if k else 0
                    chain.append((k, False, S + 1 + carry, r * S - carry, r * S - carry))
                if fw:
                    k = k_first + n_win
                    P = fids + 1 + (r * (S - H) if k else 0)
                    budget = min(max_new, block - P)
                    chain.append((k, True, P, budget, budget if final_steps is None else min(int(final_steps[i]), budget)))
            chains.append(chain)
        slot = [None] * slots       # [stream, index in its chain, running, steps sampled in the window]
        next_src = 0
        while True:
            for j in range(slots):
                if slot[j] is None:
                    while next_src < n and not chains[next_src]:
                        next_src += 1
                    if next_src < n:
                        slot[j] = [next_src, 0, False, 0]
                        placement[next_src][0] = j
                        next_src += 1
            if all(s is None for s in slot):
                break
            at = len(ticks)
            steps = [(j, s[0], chains[s[0]][s[1]][0]) for j, s in enumerate(slot) if s is not None and s[2]]
            starts, tokens = [], len(steps)
            for j, s in enumerate(slot):
                if s is None or s[2]:
                    continue
                k, final, P, _, _ = chains[s[0]][s[1]]
                if tokens + P > tick_tokens:
                    break
                starts.append((j, s[0], k, P, final))
                tokens += P
                s[2], s[3] = True, 0
                if placement[s[0]][1] < 0:
                    placement[s[0]][1] = at
            waiting = [j for j, s in enumerate(slot) if s is not None and not s[2]]
            in_final = False
            for j in [x[0] for x in steps] + [x[0] for x in starts]:
                s = slot[j]
                _, final, _, budget, _ = chains[s[0]][s[1]]
                s[3] += 1
                if s[3] < budget:
                    in_final = in_final or final
                    continue
                s[1], s[2] = s[1] + 1, False
                if s[1] >= len(chains[s[0]]):
                    placement[s[0]][2] = at
                    slot[j] = None
            ticks.append((len(steps), len(starts), tokens - len(steps), 1 if tokens > GEMM_ABOVE else 0, g))
            poll = in_final and len(ticks) % CHECK_EVERY == 0
            if poll:
                for j, s in enumerate(slot):
                    if s is not None and s[2] and chains[s[0]][s[1]][1] and s[3] >= chains[s[0]][s[1]][4]:
                        placement[s[0]][2] = at
                        slot[j] = None
            events.append((steps, starts, poll, waiting))
    placement = [tuple(p) for p in placement]
    return (rounds, ticks, placement, events) if detail else (rounds, ticks, placement)


def fine_pool_passes(streams, W: int, fine_slots: int):
    """The fine stage's part of one call (``FinePoolSchedule`` in csrc/fine.h is the same arithmetic). ``streams``: per stream of the call
    ``(frames before the call, frames handed over, final)``. Each stream's work is §25's (``fine_stream_rounds``); a round is global, and in a round wave w
    holds the w-th runnable window of every stream that has one, in passes of up to ``fine_slots`` windows, so two windows of one stream never share a
    pass. Returns ``(rounds, passes)``: per round and stream its ``fine_stream_rounds`` tuple or None, per pass ``(round, wave, [(stream, window, rel)])``."""
    per = [fine_stream_rounds(int(b), int(m), bool(f), W) for b, m, f in streams]
    rounds, passes = [], []
    for g in range(max([len(p) for p in per] + [0])):
        rd = [p[g] if g < len(p) else None for p in per]
        rounds.append(rd)
        chains = []
        for x in rd:
            chain = []
            if x is not None:
                take, first, held, j_first, n_win, pad, last, rel, e0, e1, shift = x
                chain = [(j_first + w, 0) for w in range(n_win)] + ([(j_first + n_win, rel)] if last else [])
            chains.append(chain)
        for wave in range(max([len(c) for c in chains] + [0])):
            todo = [(i, c[wave][0], c[wave][1]) for i, c in enumerate(chains) if len(c) > wave]
            for at in range(0, len(todo), fine_slots):
                passes.append((g, wave, todo[at:at + fine_slots]))
    return rounds, passes


# ---- stage 1 on its own ----------------------------------------------------------------------------------------------------------------------------------
class _GptRecord:
    """What a pool knows of one stream; readable after its flush."""

    def __init__(self, sid: int, place: int, draws: _Draws):
        self.sid, self.place, self.draws = sid, place, draws
        self.ids_in = 0
        self.length = 0                      # stream ids produced so far
        self.finish: Optional[str] = None
        self.windows: List[tuple] = []
        self.state = "open"                  # "open" | "flushed" | "closed"
        self.pieces: List[torch.Tensor] = []
        self.logit_pieces: List[torch.Tensor] = []
        self.tail: Optional[torch.Tensor] = None   # the flush's piece past the ids it produced: nothing may be written there


class GptStreamPool:
    """Stage 1 of a stream pool: ``open()`` streams, ``push({sid: ids}, flush=[sid])`` -> ``{sid: the stream's new raw ids, int32 on the
    device}``. Up to ``streams`` streams are live at once and share ``slots`` cache rows; the device state holds, per stream, only its ``2 S`` source ids
    and its carry. A stream's ids are those of ``to_acoustic_long([source], window, hop, max_new_tokens, temperature, top_k, uniforms=, top_p=, min_p=)``
    under §20's protocol: stream position p draws ``uniforms[p]`` (from ``seed``: ``Philox(seed)``, as ``audio_stream(seed=)``). With ``slots = 1`` every
    tick is a lone prefill or a lone step and the ids and logits are bit-equal to that call. ``keep_ids`` keeps what was produced (on the device) for
    ``ids_of`` / ``stream().pieces``; ``return_logits`` keeps the logits of every step. ``last_ticks`` / ``last_rounds`` / ``last_placement`` / ``last_call``
    describe the last push (``pool_schedule``'s form, and the call's ``(sid, ids before, ids pushed, flushed)`` in ascending id)."""

    def __init__(self, gpt, streams: int = 64, slots: int = 16, window: Optional[int] = None, hop: Optional[int] = None, max_new_tokens: int = 1024,
                 temperature: float = 0.8, top_k: int = 100, top_p: Optional[float] = None, min_p: Optional[float] = None, tick_tokens: Optional[int] = None,
                 keep_ids: bool = False, return_logits: bool = False):
        self._truncation = check_truncation(top_p, min_p)
        self.gpt = gpt
        cfg = gpt.config
        self.r, self.block = int(cfg.ids_per_source_token), gpt.block_size
        self.S = default_window(cfg, self.block)[0] if window is None else int(window)
        self.H = (self.S // 2) // 2 * 2 if hop is None else int(hop)
        check_windows(self.S, self.H, self.r, self.block)
        self.streams, self.slots, self.max_new = int(streams), int(slots), int(max_new_tokens)
        if not 1 <= self.streams <= MAX_POOL_STREAMS:
            raise ValueError(f"stream pool: streams must be 1 to {MAX_POOL_STREAMS}, got {self.streams}")
        if not 1 <= self.slots <= MAX_SLOTS:
            raise ValueError(f"stream pool: slots must be 1 to {MAX_SLOTS}, got {self.slots}")
        if not 1 <= self.max_new <= 1024:
            raise ValueError(f"stream pool: max_new_tokens must be 1 to 1024, got {self.max_new}")
        self.max_len = pool_max_len(self.S, self.H, self.r, self.block, self.max_new)
        self.tick_tokens = self.slots + DEFAULT_TICK_WINDOWS * self.max_len if tick_tokens is None else int(tick_tokens)
        if not self.slots + self.max_len <= self.tick_tokens <= MAX_SLOTS * 1025:
            raise ValueError(f"stream pool: tick_tokens must be at least slots + the longest window ({self.slots} + {self.max_len}) and at most "
                             f"{MAX_SLOTS * 1025}, got {self.tick_tokens}")
        self.temperature, self.top_k = float(temperature), int(top_k)
        self.keep_ids, self.return_logits = bool(keep_ids), bool(return_logits)
        self.device = gpt.device
        with torch.cuda.device(self.device):
            n = int(gpt._fn("pool_state_bytes")(gpt.handle, self.streams, self.slots, self.max_len, self.tick_tokens, self.S, self.H, self.r))
            if n == 0:
                raise ValueError(f"stream pool: {_cabi.last_error()}")
            self._state = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._pos = (C.c_int64 * (2 * self.streams))()
        self._free = list(range(self.streams))
        self._rec: Dict[int, _GptRecord] = {}
        self._next_sid = 0
        self.last_ticks: List[tuple] = []
        self.last_rounds = 0
        self.last_placement: List[tuple] = []
        self.last_call: List[tuple] = []
        self.last_out = None
        self.calls = 0   # library calls made: a refused push makes none

    @property
    def state_bytes(self) -> int:
        return self._state.numel()

    @property
    def open_streams(self) -> int:
        return self.streams - len(self._free)

    def open(self, seed: int = 0, uniforms=None) -> int:
        """A new stream; its id is never reused. ``uniforms``: explicit draws, one per stream position (tests)."""
        if not self._free:
            raise ValueError(f"stream pool: all {self.streams} streams are open")
        sid, place = self._next_sid, self._free.pop(0)
        self._next_sid += 1
        self._pos[2 * place], self._pos[2 * place + 1] = 0, 0
        self._rec[sid] = _GptRecord(sid, place, _Draws(int(seed), 1, uniforms, "uniforms"))
        return sid

    def stream(self, sid: int) -> _GptRecord:
        if sid not in self._rec:
            raise ValueError(f"stream pool: unknown stream {sid}")
        return self._rec[sid]

    def ids_of(self, sid: int) -> torch.Tensor:
        """``keep_ids``: the stream's raw ids so far, int64 on the CPU."""
        if not self.keep_ids:
            raise ValueError("stream pool: ids_of needs keep_ids=True")
        p = self.stream(sid).pieces
        return torch.cat(p).cpu().to(torch.int64) if p else torch.empty(0, dtype=torch.int64)

    def logits_of(self, sid: int) -> torch.Tensor:
        """``return_logits``: the logits of every step the stream sampled, float32 ``[n + stopped, V]`` on the CPU."""
        if not self.return_logits:
            raise ValueError("stream pool: logits_of needs return_logits=True")
        p = self.stream(sid).logit_pieces
        return torch.cat(p).cpu() if p else torch.empty((0, self.gpt.vocab), dtype=torch.float32)

    def close(self, sid: int) -> None:
        """Drop an open stream without output; its place is free for the next ``open()``."""
        rec = self.stream(sid)
        if rec.state != "open":
            raise ValueError(f"stream pool: stream {sid} is {rec.state}")
        rec.state = "closed"
        self._free.append(rec.place)
        self._free.sort()

    def flush(self, sids: Iterable[int]):
        return self.push({}, flush=sids)

    # ---- one call ------------------------------------------------------------------------------------------------------------------------------------
    def plan(self, items, flush=()):
        """Everything a push can be refused for, checked for the whole call before anything is launched or changed. Returns the call's streams in
        ascending id: ``[(record, int32 ids, final, k0, k1, new ids of the non-final windows, the final window's budget, its draws)]``."""
        cfg, S, H, r = self.gpt.config, self.S, self.H, self.r
        flush = [int(s) for s in flush]
        if len(set(flush)) != len(flush):
            raise ValueError("stream pool: a stream is flushed twice in one call")
        out = []
        for sid in sorted(set(int(s) for s in items) | set(flush)):
            rec = self._rec.get(sid)
            if rec is None:
                raise ValueError(f"stream pool: unknown stream {sid}")
            if rec.state != "open":
                raise ValueError(f"stream pool: stream {sid} is {rec.state}")
            ids = items.get(sid, ())
            t = torch.as_tensor(np.asarray(ids.cpu() if isinstance(ids, torch.Tensor) else ids)).reshape(-1)
            if t.numel() and (t.is_floating_point() or t.dtype == torch.bool):
                raise ValueError(f"stream pool: ids must be integers, got {t.dtype}")
            t = t.to(torch.int64)
            if t.numel() and (int(t.min()) < 0 or int(t.max()) >= cfg.SEMANTIC_VOCAB_SIZE):
                raise ValueError(f"stream pool: semantic ids must lie in [0, {cfg.SEMANTIC_VOCAB_SIZE})")
            n_before, n_new, final = rec.ids_in, int(t.numel()), sid in flush
            if n_before + n_new > MAX_SOURCE_IDS:
                raise ValueError(f"stream pool: a source has at most {MAX_SOURCE_IDS} ids")
            if final and n_before + n_new == 0:
                raise ValueError(f"stream pool: stream {sid} is flushed with nothing pushed")
            k0, k1 = gpt_windows_run(n_before, S, H), gpt_windows_run(n_before + n_new, S, H)
            new_ids = sum(gpt_window_ids(k, S, H, r)[1] for k in range(k0, k1))
            budget = 0
            if final:
                budget = min(self.max_new, self.block - (n_before + n_new - k1 * H + 1 + (r * (S - H) if k1 else 0)))
            u = rec.draws.rows(rec.length, rec.length + new_ids + budget).reshape(-1)   # raises where explicit draws run out
            out.append((rec, t.to(torch.int32), final, k0, k1, new_ids, budget, u))
        return out

    def push(self, items, flush=(), plan=None):
        """``plan``: what ``plan(items, flush)`` returned for this very call, when the caller has made it already."""
        call = self.plan(items, flush) if plan is None else plan
        if not call:
            return {}
        cfg, S, H, r, dev = self.gpt.config, self.S, self.H, self.r, self.device
        n = len(call)
        carry0 = [r * (S - H) if k0 else 0 for _, _, _, k0, _, _, _, _ in call]
        out_stride = max(2, max(c + new + b for c, (_, _, _, _, _, new, b, _) in zip(carry0, call)))
        out_stride += out_stride % 2          # rows stay 8-byte aligned: a frame of two ids is one load of the fine stage's hand-over
        u_stride = max(1, max(new + b for _, _, _, _, _, new, b, _ in call))
        u_host = np.zeros((n, u_stride), dtype=np.float32)
        for i, (_, _, _, _, _, new, b, u) in enumerate(call):
            u_host[i, :new + b] = u
        ids_host = torch.cat([t for _, t, *_ in call]) if any(t.numel() for _, t, *_ in call) else None
        self.last_call = [(rec.sid, rec.ids_in, int(t.numel()), final) for rec, t, final, *_ in call]
        cap_ticks = sum(new + b for _, _, _, _, _, new, b, _ in call) + CHECK_EVERY * (n + 1)
        c_trace = (C.c_int32 * (5 * cap_ticks))()
        c_ticks, c_rounds = C.c_int32(0), C.c_int32(0)
        c_place = (C.c_int32 * (3 * n))()
        c_ran = (C.c_int32 * n)()
        with torch.cuda.device(dev):
            d_ids = None if ids_host is None else ids_host.to(dev)
            d_u = torch.from_numpy(u_host).to(dev)
            d_out = torch.full((n, out_stride), -1, dtype=torch.int32, device=dev)
            d_len = torch.zeros(n, dtype=torch.int32, device=dev)
            d_fin = torch.zeros(n, dtype=torch.int32, device=dev)
            d_logits = torch.empty((n, out_stride, self.gpt.vocab), dtype=torch.float32, device=dev) if self.return_logits else None
            self.calls += 1
            with self.gpt._truncated(*self._truncation):
                _cabi.check(self.gpt._fn("pool_push")(
                    self.gpt.handle, self._state.data_ptr(), self._state.numel(), self.streams, self.slots, self.max_len, self.tick_tokens, self._pos, n,
                    (C.c_int32 * n)(*[rec.place for rec, *_ in call]), _cabi.ptr(d_ids), (C.c_int32 * n)(*[int(t.numel()) for _, t, *_ in call]),
                    (C.c_int32 * n)(*[1 if final else 0 for _, _, final, *_ in call]), S, H, r, cfg.SEMANTIC_OFFSET, cfg.SEMANTIC_VOCAB_SIZE, cfg.INFER_TOKEN,
                    cfg.ACOUSTIC_OFFSET, cfg.codebook_size, cfg.STOP_TOKEN, self.max_new, self.temperature, self.top_k, d_u.data_ptr(), u_stride,
                    (C.c_int64 * n)(*[rec.length for rec, *_ in call]), d_out.data_ptr(), out_stride, d_len.data_ptr(), d_fin.data_ptr(), _cabi.ptr(d_logits),
                    c_ran, c_trace, cap_ticks, C.byref(c_ticks), C.byref(c_rounds), c_place, _cabi.current_stream_handle(dev), self._status.data_ptr()),
                    "at_gpt_pool_push")
            self.last_ticks = [tuple(c_trace[5 * i:5 * i + 5]) for i in range(min(c_ticks.value, cap_ticks))]
            self.last_rounds = c_rounds.value
            self.last_placement = [tuple(c_place[3 * i:3 * i + 3]) for i in range(n)]
            if any(final for _, _, final, *_ in call):   # the final lengths: the call's one look at the device besides the flag polls
                lens, fins = d_len.tolist(), d_fin.tolist()
            result = {}
            for i, (rec, t, final, k0, k1, new_ids, budget, _) in enumerate(call):
                first_new = rec.length
                for k in range(k0, k1):
                    rec.windows.append((k * H, S, r * (S - H) if k else 0, gpt_window_ids(k, S, H, r)[1]))
                made, stopped = new_ids, 0
                if final:
                    total = max(lens[i], first_new + new_ids)   # the length is written with an id: a final window that stops at once writes none
                    rec.finish, stopped = FINISH[fins[i]], 1 if fins[i] == 1 else 0
                    rec.windows.append((k1 * H, rec.ids_in + int(t.numel()) - k1 * H, r * (S - H) if k1 else 0, total - first_new - new_ids))
                    made = total - first_new
                    rec.state = "flushed"
                    self._free.append(rec.place)
                    rec.tail = d_out[i, carry0[i] + made:].clone()
                piece = d_out[i, carry0[i]:carry0[i] + made]
                result[rec.sid] = piece.clone()
                if self.keep_ids and made:
                    rec.pieces.append(result[rec.sid])
                if d_logits is not None and made + stopped:
                    rec.logit_pieces.append(d_logits[i, carry0[i]:carry0[i] + made + stopped].clone())
                rec.ids_in += int(t.numel())
                rec.length += made
            self._free.sort()
            self.last_out = (d_out, out_stride, carry0)   # the call's pieces as the library wrote them: what the fine stage's hand-over reads
            if any(final for _, _, final, *_ in call) and int(self._status.item()) & 1:
                raise ValueError("stream pool: a source id lies outside the semantic vocabulary")
        return result


# ---- all three stages ----------------------------------------------------------------------------------------------------------------------------------
class _AudioRecord:
    """``pool.stream(sid)``: what a pool knows of one stream; readable after its flush."""

    def __init__(self, gpt_rec: _GptRecord, fine_draws: _Draws, place: int, dsid: int, keep_codes: bool, return_logits: bool, acoustic_offset: int, vocab: int):
        self._g, self._fu, self.place, self._dsid = gpt_rec, fine_draws, place, dsid
        self._keep, self._logits_on, self._offset, self._vocab = keep_codes, return_logits, acoustic_offset, vocab
        self.frames_in = self.frames_out = 0
        self.fine_windows_run: List[tuple] = []
        self._codes: List[torch.Tensor] = []

    ids_in = property(lambda self: self._g.ids_in)
    finish = property(lambda self: self._g.finish)
    windows = property(lambda self: list(self._g.windows))
    state = property(lambda self: self._g.state)

    def _kept(self):
        if not self._keep:
            raise ValueError("audio_stream_pool: coarse_ids / fine_codes need keep_codes=True")

    @property
    def coarse_ids(self) -> torch.Tensor:
        self._kept()
        p = self._g.pieces
        return (torch.cat(p).cpu().to(torch.int64) if p else torch.empty(0, dtype=torch.int64)) - self._offset

    @property
    def fine_codes(self) -> torch.Tensor:
        self._kept()
        return torch.cat(self._codes, dim=1).cpu() if self._codes else torch.empty((8, 0), dtype=torch.int64)

    @property
    def logits(self) -> torch.Tensor:
        if not self._logits_on:
            raise ValueError("audio_stream_pool: logits need return_logits=True")
        p = self._g.logit_pieces
        return torch.cat(p).cpu() if p else torch.empty((0, self._vocab), dtype=torch.float32)


class SemanticAudioStreamPool:
    """``AudioToken.audio_stream_pool()``: up to ``streams`` live semantic-to-audio streams on one device state. ``sid = open(seed=)``;
    ``push({sid: ids}, flush=[sid]) -> {sid: float32 (1, 320 n) on the CPU}`` for every stream named (``n`` may be 0); ``flush(sids)``; ``close(sid)``;
    ``stream(sid)`` is the stream's record. A stream opened with seed ``s`` is ``audio_stream(seed=s)`` pushed the same ids: the same GPT windows, fine
    windows and draws, frames leaving in the call in which they turn final. The streams share ``slots`` GPT cache rows (``GptStreamPool``), the fine
    stage's passes of up to ``fine_slots`` windows (``at_fine_pool_push``) and one ``decode_stream_pool(slots=streams)``. One call is checked whole
    before anything is launched; explicit ``fine_uniforms`` of a flushed stream must cover the longest the stream can get (its final window's whole
    budget), since only the device knows its length. A flushed stream with no whole frame raises ``to_audio``'s error once the other streams of the call
    are complete, and their audio is in ``last_output``."""

    def __init__(self, gpt, fine, decode_pool, streams: int = 64, slots: int = 16, fine_slots: int = 4, window: Optional[int] = None, hop: Optional[int] = None,
                 max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100, top_p: Optional[float] = None, min_p: Optional[float] = None,
                 fine_temperature: Optional[float] = 0.5, tick_tokens: Optional[int] = None, keep_codes: bool = False, return_logits: bool = False, voice=None):
        if voice is not None:
            raise ValueError("audio_stream: voice= is not built for streams (the prompted schedule changes every window); use to_audio(long_form=True, voice=)")
        self.gpt_pool = GptStreamPool(gpt, streams=streams, slots=slots, window=window, hop=hop, max_new_tokens=max_new_tokens, temperature=temperature,
                                      top_k=top_k, top_p=top_p, min_p=min_p, tick_tokens=tick_tokens, keep_ids=keep_codes, return_logits=return_logits)
        self.gpt, self.fine, self._decode = gpt, fine, decode_pool
        self.streams, self.fine_slots, self.W = int(streams), int(fine_slots), fine.block_size
        if not 1 <= self.fine_slots <= 64:
            raise ValueError(f"audio_stream_pool: fine_slots must be 1 to 64, got {self.fine_slots}")
        self.fine_temperature, self.keep_codes, self.return_logits = fine_temperature, bool(keep_codes), bool(return_logits)
        self.device = gpt.device
        with torch.cuda.device(self.device):
            n = int(fine._fn("pool_state_bytes")(fine.handle, self.streams, self.fine_slots))
            if n == 0:
                raise ValueError(f"audio_stream_pool: {_cabi.last_error()}")
            self._fine_state = torch.empty(n, dtype=torch.uint8, device=self.device)
            self._status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._fpos = (C.c_int64 * (2 * self.streams))()
        self._rec: Dict[int, _AudioRecord] = {}
        self._by_dsid: Dict[int, int] = {}
        self.last_output: Dict[int, torch.Tensor] = {}
        self.last_fine_passes: List[tuple] = []

    @property
    def state_bytes(self):
        """``(GPT state, fine state)`` in bytes: fixed by the capacities, the geometry and the models, whatever the sources' lengths."""
        return self.gpt_pool.state_bytes, self._fine_state.numel()

    def open(self, seed: int = 0, uniforms=None, fine_uniforms=None) -> int:
        if fine_uniforms is not None and np.shape(fine_uniforms)[1:] != (N_PASSES, self.W):
            raise ValueError(f"fine_uniforms must be float32 [n, {N_PASSES}, {self.W}] (window, code book, buffer position), got {np.shape(fine_uniforms)}")
        sid = self.gpt_pool.open(seed=seed, uniforms=uniforms)   # raises when all streams are open
        g = self.gpt_pool.stream(sid)
        self._fpos[2 * g.place], self._fpos[2 * g.place + 1] = 0, 0
        rec = _AudioRecord(g, _Draws(int(seed), N_PASSES * self.W, fine_uniforms, "fine_uniforms"), g.place, self._decode.open(), self.keep_codes,
                           self.return_logits, self.gpt.config.ACOUSTIC_OFFSET, self.gpt.vocab)
        self._rec[sid] = rec
        self._by_dsid[rec._dsid] = sid
        return sid

    def stream(self, sid: int) -> _AudioRecord:
        if sid not in self._rec:
            raise ValueError(f"audio_stream_pool: unknown stream {sid}")
        return self._rec[sid]

    def close(self, sid: int) -> None:
        self.gpt_pool.close(sid)
        self._decode.close(self._rec[sid]._dsid)

    def flush(self, sids: Iterable[int]):
        return self.push({}, flush=sids)

    def _fine_plan(self, rec: _AudioRecord, n_frames: int, final: bool, greedy: bool):
        """What the fine stage does with ``n_frames`` more frames of one stream: (its windows' draws ``[n, 6 W]`` or None, the first window, the frames
        that turn final, the windows as ``(start, fill)``). Raises where explicit draws run out."""
        W, H = self.W, self.W // 2
        wins, n_emit, j_lo, j_hi = [], 0, None, None
        T = rec.frames_in + n_frames
        for take, first, held, j_first, n_win, pad, last, rel, e0, e1, shift in fine_stream_rounds(rec.frames_in, n_frames, final, W):
            wins += [(j * H, j * H) for j in range(j_first, j_first + n_win)]
            if last:
                wins.append((T - W, T - W + rel))
            if n_win + last:
                j_lo, j_hi = (j_first if j_lo is None else j_lo), j_first + n_win + last
            n_emit += e1 - e0
        fu = rec._fu.rows(j_lo, j_hi) if wins and not greedy else None
        return fu, (j_lo or 0), n_emit, wins

    def push(self, items, flush=()):
        gp, cfg, dev = self.gpt_pool, self.gpt.config, self.device
        greedy = self.fine_temperature is None
        flush = list(flush)
        call = gp.plan(items, flush)     # every refusal of stage 1, for the whole call
        # The fine stage's part of every stream that is not flushed is known now. A flushed stream's length is the device's to decide, within its final
        # window's budget, and the windows of a row only grow with its length: its explicit draws must cover the longest it can get. So explicit draws
        # that run out are refused here, for the whole call, before anything is launched, and nothing after stage 1 can refuse a stream for its draws.
        plans = {}
        for rec_g, _, final, _, _, new_ids, budget, _ in call:
            rec = self._rec[rec_g.sid]
            if not final:
                plans[rec_g.sid] = self._fine_plan(rec, (rec_g.length + new_ids) // 2 - rec.frames_in, False, greedy)
            elif (rec_g.length + new_ids + budget) // 2 >= 1:
                self._fine_plan(rec, (rec_g.length + new_ids + budget) // 2 - rec.frames_in, True, greedy)
        if not call:
            return {}
        gp.push(items, flush, plan=call)
        d_out, out_stride, carry0 = gp.last_out
        out, bad, todo = {}, [], []
        for i, (rec_g, _, final, *_) in enumerate(call):
            sid, rec = rec_g.sid, self._rec[rec_g.sid]
            n_frames = rec_g.length // 2 - rec.frames_in
            if final:
                if rec_g.length // 2 < 1:
                    bad.append(sid)
                    self._decode.close(rec._dsid)
                    self._fpos[2 * rec.place + 1] = 1
                    continue
                plans[sid] = self._fine_plan(rec, n_frames, True, greedy)   # covered by the check before the launch
            assert carry0[i] + 2 * n_frames <= out_stride, "the frames handed over are this call's ids"
            if n_frames or final:
                todo.append((i, sid, rec, n_frames, final))
            else:
                out[sid] = torch.empty((1, 0), dtype=torch.float32)
        pieces = {}
        if todo:
            n = len(todo)
            fus = [plans[sid][0] for _, sid, *_ in todo]
            cells = np.cumsum([0] + [0 if fu is None else fu.shape[0] for fu in fus])
            emit_stride = max(1, max(plans[sid][2] for _, sid, *_ in todo))
            c_emit, c_ran, c_passes = (C.c_int32 * n)(), (C.c_int32 * n)(), C.c_int32(0)
            cap = sum(len(plans[sid][3]) for _, sid, *_ in todo) + 1
            c_trace = (C.c_int32 * (3 * cap))()
            with torch.cuda.device(dev):
                d_fu = None
                if cells[-1]:
                    d_fu = torch.from_numpy(np.ascontiguousarray(np.concatenate([fu for fu in fus if fu is not None]))).to(dev)
                d_emit = torch.empty((n, 8, emit_stride), dtype=torch.int64, device=dev)
                _cabi.check(self.fine._fn("pool_push")(
                    self.fine.handle, self._fine_state.data_ptr(), self._fine_state.numel(), self.streams, self.fine_slots, self._fpos, n,
                    (C.c_int32 * n)(*[rec.place for _, _, rec, _, _ in todo]), d_out.data_ptr(),
                    (C.c_int64 * n)(*[i * out_stride + carry0[i] for i, *_ in todo]), (C.c_int32 * n)(*[m for *_, m, _ in todo]),
                    (C.c_int32 * n)(*[1 if f else 0 for *_, f in todo]), cfg.ACOUSTIC_OFFSET, cfg.codebook_size, 1.0 if greedy else float(self.fine_temperature),
                    1 if greedy else 0, _cabi.ptr(d_fu), (C.c_int32 * n)(*[int(c) for c in cells[:-1]]), (C.c_int32 * n)(*[plans[sid][1] for _, sid, *_ in todo]),
                    (C.c_int32 * n)(*[0 if fu is None else fu.shape[0] for fu in fus]), d_emit.data_ptr(), emit_stride, c_emit, c_ran, c_trace, cap,
                    C.byref(c_passes), _cabi.current_stream_handle(dev), self._status.data_ptr()), "at_fine_pool_push")
            self.last_fine_passes = [tuple(c_trace[3 * k:3 * k + 3]) for k in range(min(c_passes.value, cap))]
            for x, (i, sid, rec, n_frames, final) in enumerate(todo):
                n_emit = plans[sid][2]
                assert c_emit[x] == n_emit, (c_emit[x], n_emit)
                rec.frames_in += n_frames
                rec.fine_windows_run.extend(plans[sid][3])
                if n_emit:
                    pieces[sid] = d_emit[x, :, :n_emit].contiguous()
                    if self.keep_codes:
                        rec._codes.append(pieces[sid].clone())
        # one decode pool for all streams: the pieces of this call, then the flushes
        audio = {sid: [] for _, sid, *_ in todo}
        if pieces:
            for sid, a in self._decode.push({self._rec[sid]._dsid: p for sid, p in pieces.items()}).items():
                audio[self._by_dsid[sid]].append(a)
        finals = [sid for _, sid, _, _, final in todo if final]
        if finals:
            for sid, a in self._decode.flush([self._rec[sid]._dsid for sid in finals]).items():
                audio[self._by_dsid[sid]].append(a)
            if int(self._status.item()) & 4:
                raise ValueError("audio_stream_pool: a stream id lies outside its code book")
        for sid, parts in audio.items():
            a = torch.cat([p.reshape(1, -1) for p in parts], dim=-1).cpu() if parts else torch.empty((1, 0), dtype=torch.float32)
            self._rec[sid].frames_out += a.shape[-1] // HOP_SAMPLES
            out[sid] = a
        self.last_output = out
        if bad:
            raise ValueError(f"to_audio: source {bad[0]} produced no whole frame of coarse codes (finish: {self._rec[bad[0]].finish})")
        return out
