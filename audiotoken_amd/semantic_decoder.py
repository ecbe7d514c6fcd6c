"""Semantic ids -> the two coarse EnCodec code books: stage 1 of the reference's semantic decoders (``gpt2_model.py``, ``decoder.py:210-239``) on the
KV-cached HIP GPT (csrc/gpt.hip). The fine stage (bark, code books 3 to 8) is fine_decoder.py; the ``[2, T]`` this stage yields is what
it takes, or what the acoustic decoder at ``num_codebooks=2`` turns into audio. The semantic ``decode`` stays absent: ``AudioToken.to_audio`` is its form here.
``to_acoustic`` keeps the first ``max_source_tokens`` ids of a source, as the reference does; ``to_acoustic_long`` walks a whole source in windows that carry the
acoustic ids of their overlap (``acoustic_windows``).

Stated deviations from the reference: the draws come from a caller-visible uniform stream, not ``torch.multinomial``; a row whose length
reaches the model's block finishes with ``"block_size"`` instead of having its context cropped; bias-free checkpoints only."""
from __future__ import annotations

import contextlib
import ctypes as C
import os
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Union

import numpy as np
import torch

from . import _cabi
from ._handle import LibHandle
from .configs import HubertDecoderConfig

FINISH = {1: "stop", 2: "max_new_tokens", 3: "block_size"}


@dataclass
class AcousticGeneration:
    """What ``to_acoustic`` returns, one entry per row of the batch."""
    ids: List[torch.Tensor]                 # int64 [n_b]: the generated ids minus the acoustic offset (the stop token is not among them)
    codes: List[Optional[torch.Tensor]]     # int64 [2, n_b // 2], or None where ``coarse_codes`` refused the ids
    finish: List[str]                       # "stop" | "max_new_tokens" | "block_size"
    logits: Optional[List[torch.Tensor]] = None   # return_logits: float32 [n_b (+ 1 when the row stopped), V], the logits each id was drawn from
    windows: Optional[List[List[tuple]]] = None   # the long form: per row (source_start, source_len, carry, new_ids) of every window
    ticks: Optional[List[tuple]] = None           # the queue (``slots=``): per tick (step tokens, windows started, prefill tokens, route)
    placement: Optional[List[tuple]] = None       # the queue: per source (slot, first tick, last tick)


def coarse_codes(ids, codebook_size: int = 1024, num_codebooks: int = 2) -> torch.Tensor:
    """Offset-free acoustic ids, interleaved as the reference serialises them, -> ``[2, T]``: even positions are code book 0, odd positions minus 1024
    are code book 1. A trailing unpaired id is dropped. An id outside its code book's range raises ``ValueError`` naming the position."""
    assert num_codebooks == 2, "stage 1 produces the two coarse code books"
    ids = torch.as_tensor(ids, dtype=torch.int64).reshape(-1)
    T = ids.numel() // 2
    pairs = ids[:2 * T].reshape(T, 2) - torch.tensor([0, codebook_size])
    bad = ((pairs < 0) | (pairs >= codebook_size)).reshape(-1).nonzero()
    if bad.numel():
        pos = int(bad[0])
        raise ValueError(f"coarse_codes: id {int(ids[pos])} at position {pos} is outside code book {pos % 2}'s range "
                         f"[{(pos % 2) * codebook_size}, {(pos % 2 + 1) * codebook_size})")
    return pairs.t().contiguous()


def source_ids(tokens, config: HubertDecoderConfig) -> torch.Tensor:
    """One source as flat int64 semantic ids: a tensor / array / path, any shape. Empty sources and ids outside the semantic vocabulary raise."""
    if isinstance(tokens, (str, os.PathLike, Path)):
        p = str(tokens)
        tokens = np.load(p) if p.endswith(".npy") else torch.load(p, map_location="cpu")
    t = torch.as_tensor(np.asarray(tokens.cpu() if isinstance(tokens, torch.Tensor) else tokens)).to(torch.int64).reshape(-1)
    if t.numel() == 0:
        raise ValueError("to_acoustic: an empty source")
    if int(t.min()) < 0 or int(t.max()) >= config.SEMANTIC_VOCAB_SIZE:
        raise ValueError(f"to_acoustic: semantic ids must lie in [0, {config.SEMANTIC_VOCAB_SIZE})")
    return t


def prepare_source(tokens, config: HubertDecoderConfig) -> np.ndarray:
    """The prompt of one source, as the reference's ``_prepare_source`` builds it: ids + the semantic offset, flattened, truncated to
    ``max_source_tokens``, the INFER token appended."""
    t = (source_ids(tokens, config) + config.SEMANTIC_OFFSET)[:config.max_source_tokens]
    return np.concatenate([t.numpy(), [config.INFER_TOKEN]]).astype(np.int32)


MAX_SOURCE_IDS = 65536   # of one row of the long form (csrc/gpt.h: GPT_MAX_SOURCE)


def check_windows(S: int, H: int, r: int, block: int) -> None:
    """The long form's conditions on window ``S``, hop ``H`` and ``r`` acoustic ids per source id at a model of ``block`` positions."""
    if S < 2 or H < 2 or S % 2 or H % 2:
        raise ValueError(f"long form: the window ({S}) and the hop ({H}) must be even, at least 2")
    if H > S:
        raise ValueError(f"long form: the hop ({H}) must not exceed the window ({S})")
    if r < 1 or S + 1 + r * S > block:
        raise ValueError(f"long form: a window of {S} source ids needs {S} + 1 + {r} * {S} positions, the model has {block}")


def default_window(config: HubertDecoderConfig, block: int):
    """``(S, H)``: the largest even window that fits the source limit and the block with its ``r S`` new ids, and the largest even hop up to half of it."""
    r = config.ids_per_source_token
    S = min(config.max_source_tokens, (block - 1) // (r + 1)) // 2 * 2
    return S, (S // 2) // 2 * 2


def check_prompt(P: int, N: int, S: int, H: int) -> None:
    """What a voice prompt of ``P`` ids in front of a source of ``N`` must satisfy (``gpt_voice_prompt_ok`` in csrc/gpt.h)."""
    if P < 2 or P % 2 or P > S - H:
        raise ValueError(f"voice prompt: its length ({P}) must be even, 2 to window - hop ({S - H})")
    if N < 1 or P + N > MAX_SOURCE_IDS:
        raise ValueError(f"voice prompt: the prompt and the source have 1 + 2 to {MAX_SOURCE_IDS} ids together, got {P} + {N}")


def acoustic_windows(N: int, S: int, H: int, r: int = 3, block: int = 1024, prompt: int = 0):
    """The long form's schedule for a source of ``N`` ids (csrc/gpt.h has the same arithmetic): a list of
    ``(source_start, source_len, carry, new_ids)``, one per window. Window k reads source ids ``[k H, k H + source_len)``, is prompted with the ``carry``
    stream ids ``[r k H, r k H + carry)`` the window before produced, and produces exactly ``new_ids`` ids from stream position ``r k H + carry`` on;
    ``new_ids`` of the last window is None: it runs until STOP or its budget.
    After a voice prompt of ``prompt`` ids the schedule is that of the concatenated source, prompt ids then the ``N`` source ids, and all
    positions are the concatenated source's and its stream's: window 0 carries the prompt's ``r * prompt`` given ids, stream positions ``[0, r * prompt)``."""
    check_windows(S, H, r, block)
    if N < 1 or N > MAX_SOURCE_IDS:
        raise ValueError(f"long form: a source has 1 to {MAX_SOURCE_IDS} ids, got {N}")
    if prompt:
        check_prompt(prompt, N, S, H)
    M = prompt + N
    n = 1 if M <= S else -(-(M - S) // H) + 1
    out = []
    for k in range(n):
        carry = r * (S - H) if k else r * prompt
        out.append((k * H, min(S, M - k * H), carry, None if k == n - 1 else r * S - carry))
    return out


MAX_QUEUE_SOURCES = 4096   # of one queue call (csrc/gpt.h: GPT_MAX_QUEUE)
MAX_SLOTS = 64             # cache rows (GPT_MAX_B)
CHECK_EVERY = 16           # ticks between two looks of the host at the slots' flags (GPT_CHECK_EVERY)
GEMM_ABOVE = 64            # a tick of more tokens takes the GEMM route (GPT_GEMM_ABOVE)
DEFAULT_TICK_WINDOWS = 2   # the default tick_tokens is slots + this many windows of max_len


def window_steps(plan, max_new: int, block: int):
    """Per window of ``acoustic_windows``' plan: (prompt tokens, steps); the final window's steps are its budget."""
    out = []
    for start, n_src, carry, new in plan:
        P = n_src + 1 + carry
        out.append((P, min(max_new, block - P) if new is None else new))
    return out


def stream_extent(plans, S: int, r: int, max_new: int, block: int, prompts=None):
    """What a set of sources needs, from their ``acoustic_windows`` plans (``gpt_extent`` in csrc/gpt.h is the same arithmetic): ``(base, cap, longest)``,
    per source the stream position of its final window's step 0, the ids of the longest source's stream, and the positions of the longest window with
    its new ids (a non-final window fills ``S + 1 + r S``). ``prompts``: per source its voice prompt's length; ``base`` and ``cap`` count RESULT positions,
    stream positions minus ``r`` times that length."""
    base, cap, longest = [], 0, 0
    for i, plan in enumerate(plans):
        start, _, carry, _ = plan[-1]
        P, budget = window_steps(plan, max_new, block)[-1]
        base.append(r * start + carry - r * (prompts[i] if prompts else 0))
        cap = max(cap, base[-1] + budget)
        longest = max(longest, P + budget, S + 1 + r * S if len(plan) > 1 else 0)
    return base, cap, longest


def queue_ticks(lens, S: int, H: int, r: int, block: int, max_new: int, slots: int, tick_tokens: int, final_steps=None, detail: bool = False, prompts=None):
    """The generation queue's host scheduler (``GptQueueSchedule`` in csrc/gpt.h is the same arithmetic): sources of ``lens`` ids run §19's
    windows through ``slots`` cache rows. Waiting sources take empty slots in source order. A tick holds one step token of every slot that is mid-window
    and the whole prompt of every window admitted, in slot order, while the list stays within ``tick_tokens``; the first window that does not fit waits,
    and so does every slot after it. Every slot with a token samples once. A non-final window ends after its exact count and a final one after its budget,
    which the host knows; a final window that ends earlier (``final_steps[i]`` sampler launches: its new ids, plus one for a sampled STOP) is seen at the
    next poll, every ``CHECK_EVERY`` ticks while some slot is in a final window, and keeps stepping until then. Returns ``(ticks, placement)``: per tick
    ``(step tokens, windows started, prefill tokens, route)`` with route 1 above ``GEMM_ABOVE`` tokens, per source ``(slot, first tick, last tick)``.
    ``detail``: a third list, per tick ``(steps [(slot, source, window)], starts [(slot, source, window, prompt tokens)], polled, slots whose window waits)``."""
    n_src = len(lens)
    plans = [window_steps(acoustic_windows(int(N), S, H, r, block, prompts[i] if prompts else 0), max_new, block) for i, N in enumerate(lens)]
    if not 1 <= slots <= MAX_SLOTS or not 1 <= n_src <= MAX_QUEUE_SOURCES:
        raise ValueError(f"queue: 1 to {MAX_SLOTS} slots and 1 to {MAX_QUEUE_SOURCES} sources, got {slots} and {n_src}")
    if tick_tokens < slots + max(P for plan in plans for P, _ in plan):
        raise ValueError(f"queue: tick_tokens ({tick_tokens}) must hold a step of every slot and one whole window")
    ends = [plan[-1][1] if final_steps is None else min(int(final_steps[i]), plan[-1][1]) for i, plan in enumerate(plans)]
    slot = [None] * slots          # [source, window, running, steps sampled in the window]
    placement = [[-1, -1, -1] for _ in range(n_src)]
    ticks, events, next_src = [], [], 0
    while True:
        for j in range(slots):
            if slot[j] is None and next_src < n_src:
                slot[j] = [next_src, 0, False, 0]
                placement[next_src][0] = j
                next_src += 1
        if all(s is None for s in slot):
            break
        at = len(ticks)
        steps = [(j, s[0], s[1]) for j, s in enumerate(slot) if s is not None and s[2]]
        starts, tokens = [], len(steps)
        for j, s in enumerate(slot):
            if s is None or s[2]:
                continue
            P = plans[s[0]][s[1]][0]
            if tokens + P > tick_tokens:
                break
            starts.append((j, s[0], s[1], P))
            tokens += P
            s[2], s[3] = True, 0
            if s[1] == 0:
                placement[s[0]][1] = at
        waiting = [j for j, s in enumerate(slot) if s is not None and not s[2]]
        in_final = False
        for j in [x[0] for x in steps] + [x[0] for x in starts]:
            s = slot[j]
            final = s[1] == len(plans[s[0]]) - 1
            s[3] += 1
            if s[3] < plans[s[0]][s[1]][1]:
                in_final = in_final or final
            elif final:
                placement[s[0]][2] = at
                slot[j] = None
            else:
                s[1], s[2] = s[1] + 1, False
        ticks.append((len(steps), len(starts), tokens - len(steps), 1 if tokens > GEMM_ABOVE else 0))
        poll = in_final and len(ticks) % CHECK_EVERY == 0
        if poll:
            for j, s in enumerate(slot):
                if s is not None and s[2] and s[1] == len(plans[s[0]]) - 1 and s[3] >= ends[s[0]]:
                    placement[s[0]][2] = at
                    slot[j] = None
        events.append((steps, starts, poll, waiting))
    placement = [tuple(p) for p in placement]
    return (ticks, placement, events) if detail else (ticks, placement)


def queue_tick_bound(lens, S: int, H: int, r: int, block: int, max_new: int, prompts=None) -> int:
    """No queue call runs more ticks than this, whatever ``slots``, ``tick_tokens`` and the final windows do: every tick either samples a step some window
    still needs (there are at most the windows' budgets of those) or holds only finished slots the host has not seen, which lasts less than ``CHECK_EVERY``
    ticks per source."""
    return sum(sum(n for _, n in window_steps(acoustic_windows(int(N), S, H, r, block, prompts[i] if prompts else 0), max_new, block)) + CHECK_EVERY - 1
               for i, N in enumerate(lens))


@dataclass
class AcousticScore:
    """What ``score_acoustic`` returns, one entry per source."""
    logprob: List[torch.Tensor]             # float32 [2 T_b (+ 1 with include_stop)]: the log-probability of the id at each stream position, STOP last
    rank: List[torch.Tensor]                # int32, the same shape: ids the model puts above it (top_k = k keeps the id exactly when rank < k)
    nll: List[float]                        # the mean of -logprob over the source's scored ids, in float64 on the host
    windows: Optional[List[List[tuple]]] = None   # the long form: per source (source_start, source_len, carry, scored ids) of every window
    logits: Optional[List[torch.Tensor]] = None   # return_logits: float32 [the same count, V], the logits each id was scored on


MAX_SCORE_SOURCES = 4096   # of one score_acoustic call
MAX_SCORE_ROWS = 65536     # of one at_gpt_score call


def acoustic_stream(codes, config: HubertDecoderConfig) -> np.ndarray:
    """Integer ``[K >= 2, T]`` codes -> the ``2 T`` model ids of the stream the GPT writes: ``c0[0] + ACOUSTIC_OFFSET, c1[0] + ACOUSTIC_OFFSET + 1024,
    c0[1] + ...``, rows 0 and 1 only. The inverse of ``coarse_codes`` (which takes the ids minus the offset)."""
    c = torch.as_tensor(np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes))
    if c.dim() != 2 or c.shape[0] < 2 or c.is_floating_point() or c.dtype == torch.bool:
        raise ValueError(f"score_acoustic: codes must be integer [K >= 2, T], got {tuple(c.shape)} {c.dtype}")
    c = c[:2].to(torch.int64)
    if c.numel() and (int(c.min()) < 0 or int(c.max()) >= config.codebook_size):
        raise ValueError(f"score_acoustic: codes must lie in [0, {config.codebook_size})")
    return (c + torch.tensor([[0], [config.codebook_size]]) + config.ACOUSTIC_OFFSET).t().reshape(-1).numpy()


def refuse_long_source(n: int, config: HubertDecoderConfig) -> None:
    """The short form's limit on a source of ``n`` ids: generation cuts a longer one, and a cut here would score the wrong pairing."""
    if n > config.max_source_tokens:
        raise ValueError(f"score_acoustic: a source of {n} ids exceeds max_source_tokens ({config.max_source_tokens}); long_form=True scores it in windows")


def score_row(tokens, stream, config: HubertDecoderConfig, block: int, include_stop: bool = True):
    """The short form's row of one source: ``(sequence, score_from)``, the prompt ``to_acoustic`` builds (ids + SEMANTIC_OFFSET, INFER), then the stream's
    ids, then STOP with ``include_stop``; ``score_from`` is the first acoustic position. A source longer than ``max_source_tokens`` is refused (generation
    cuts it; a cut here would score the wrong pairing), and so is a sequence longer than the block."""
    src = source_ids(tokens, config)
    refuse_long_source(int(src.numel()), config)
    stream = np.asarray(stream, dtype=np.int64).reshape(-1)
    if stream.size % 2:
        raise ValueError(f"score_acoustic: an odd id count ({stream.size}): the stream holds whole frames of two ids")
    tail = [config.STOP_TOKEN] if include_stop else []
    seq = np.concatenate([src.numpy() + config.SEMANTIC_OFFSET, [config.INFER_TOKEN], stream, tail]).astype(np.int32)
    if seq.size > block:
        raise ValueError(f"score_acoustic: the sequence ({src.numel()} + 1 + {stream.size + len(tail)} ids) is longer than the model's block ({block})")
    if stream.size + len(tail) == 0:
        raise ValueError("score_acoustic: nothing to score: no codes and no STOP")
    return seq, int(src.numel()) + 1


def long_score_rows(tokens, stream, S: int, H: int, config: HubertDecoderConfig, block: int, include_stop: bool = True):
    """The long form's rows of one source: one per window of ``acoustic_windows``, as ``(sequence, score_from, stream position of the
    first target)``, and the schedule with the counts scored. Window k: its source ids + the offset, INFER, the ``carry`` ids the given stream holds at
    ``[r k H, r k H + carry)``, then its targets: the ``new_ids`` stream ids from ``r k H + carry`` on, for the final window everything that is left, then
    STOP with ``include_stop``. A final window with nothing to score has no row."""
    r = int(config.ids_per_source_token)
    src = source_ids(tokens, config).numpy()
    stream = np.asarray(stream, dtype=np.int64).reshape(-1)
    plan = acoustic_windows(int(src.size), S, H, r, block)
    if stream.size % 2:
        raise ValueError(f"score_acoustic: an odd id count ({stream.size}): the stream holds whole frames of two ids")
    start, n_src, carry, _ = plan[-1]
    first = r * start + carry
    P, budget = window_steps(plan, 1024, block)[-1]
    if stream.size < first:
        raise ValueError(f"score_acoustic: a stream of {stream.size} ids is shorter than the final window's first step ({first}) for a source of {src.size} ids")
    if stream.size > first + budget:
        raise ValueError(f"score_acoustic: a stream of {stream.size} ids is longer than the final window's first step plus its budget ({first} + {budget})")
    rows, windows = [], []
    for k, (start, n_src, carry, new) in enumerate(plan):
        base = r * start + carry
        final = new is None
        targets = stream[base:] if final else stream[base:base + new]
        tail = [config.STOP_TOKEN] if final and include_stop else []
        windows.append((start, n_src, carry, int(targets.size)))
        if targets.size + len(tail) == 0:
            continue
        seq = np.concatenate([src[start:start + n_src] + config.SEMANTIC_OFFSET, [config.INFER_TOKEN], stream[r * start:base], targets, tail]).astype(np.int32)
        if seq.size > block:
            raise ValueError(f"score_acoustic: the final window's sequence ({seq.size} ids with STOP) is longer than the model's block ({block}); "
                             "a stream that fills its budget did not stop: include_stop=False")
        rows.append((seq, n_src + 1 + carry, base))
    return rows, windows


def constrained_allow(config: HubertDecoderConfig):
    """The allow sets ``to_acoustic(constrain=True)`` draws under: even steps code book 0 or STOP, odd steps code book 1."""
    a, n = config.ACOUSTIC_OFFSET, config.codebook_size
    return [[a, a + n, config.STOP_TOKEN, config.STOP_TOKEN + 1], [a + n, a + 2 * n, 0, 0]]


def seeded_uniforms(seed: int, batch: int, max_new_tokens: int) -> np.ndarray:
    return np.random.Generator(np.random.Philox(seed)).random((batch, max_new_tokens), dtype=np.float32)


def check_truncation(top_p=None, min_p=None):
    """``(top_p, min_p)`` as the library takes them: ``top_p`` None or 1 is off (1.0), ``min_p`` None or 0 is off (0.0). NaN, ``top_p``
    outside (0, 1] and ``min_p`` outside [0, 1) raise ``ValueError`` before anything reaches the device."""
    p = 1.0 if top_p is None else float(top_p)
    q = 0.0 if min_p is None else float(min_p)
    if not 0.0 < p <= 1.0:
        raise ValueError(f"top_p must lie in (0, 1] (None or 1: off), got {top_p!r}")
    if not 0.0 <= q < 1.0:
        raise ValueError(f"min_p must lie in [0, 1) (None or 0: off), got {min_p!r}")
    return p, q


class SemanticToAcoustic(LibHandle):
    """Owner of one ``at_gpt`` handle. ``weights``: a checkpoint path, a ``{name: array}`` dict, or None for the seeded synthetic model."""

    FAMILY = "gpt"

    def __init__(self, config: Optional[HubertDecoderConfig] = None, device="cuda:0", weights: Union[None, str, os.PathLike, Dict[str, np.ndarray]] = None):
        self.config = config or HubertDecoderConfig()
        if weights is None:
            weights = self.config.weights

        def host_tensors():
            from . import weights as W
            if weights is None:
                return W.synth_gpt_weights(vocab=self.config.VOCAB_SIZE)
            if isinstance(weights, dict):
                return W.gpt_tensors_from_state_dict(weights, "weights dict")
            return W.read_gpt_checkpoint(weights)

        self._create(device, None, host_tensors)

    def _finish_init(self) -> None:
        self.n_layers = self._fn("num_layers")(self.handle)
        self.vocab = self._fn("vocab")(self.handle)
        self.block_size = self._fn("block_size")(self.handle)
        self._init_call_state()

    def eval(self):
        return self

    def generate(self, prompts: Sequence[np.ndarray], max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100,
                 stop_token: int = -1, uniforms: Optional[np.ndarray] = None, seed: int = 0, allow=None, return_logits: bool = False,
                 top_p: Optional[float] = None, min_p: Optional[float] = None):
        """Raw generation over the model's own vocabulary: ``prompts`` a list of int id arrays (1 to 64 rows of their own lengths). Returns
        ``(ids, finish, logits)``: per row the int64 ids on the CPU, the finish reason's name and (``return_logits``) the float32 logits
        ``[n + stopped, V]``. ``allow``: None or int ``[2][4]``, the id ranges even / odd steps may produce (include/audiotoken_hip.h).
        ``top_p`` / ``min_p``: the nucleus and the min-p cut after the top-k; None: off."""
        truncation = check_truncation(top_p, min_p)
        B = len(prompts)
        max_new = int(max_new_tokens)
        lens = [int(len(p)) for p in prompts]
        if uniforms is None:
            uniforms = seeded_uniforms(seed, B, max_new)
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float32)
        if uniforms.shape != (B, max_new):
            raise ValueError(f"uniforms must be float32 [{B}, {max_new}] (one draw per row and step), got {uniforms.shape}")
        stride = max(lens) if lens else 1
        host = np.zeros((max(B, 1), max(stride, 1)), dtype=np.int32)
        for b, p in enumerate(prompts):
            host[b, :lens[b]] = np.asarray(p, dtype=np.int32)
        max_len = max(1, min(self.block_size, stride + max_new))
        c_lens = (C.c_int32 * max(B, 1))(*lens)
        c_allow = None if allow is None else (C.c_int32 * 8)(*[int(v) for v in np.asarray(allow).reshape(8)])

        def call(dev, d_prompts, d_u, d_ids, d_len, d_fin, d_logits):
            nbytes = int(self._fn("state_bytes")(self.handle, B, max_len))
            state = self._workspace(max(nbytes, 256))
            self._status.zero_()
            _cabi.check(self._fn("generate")(self.handle, d_prompts.data_ptr(), stride, c_lens, B, max_new, float(temperature), int(top_k), int(stop_token),
                                             d_u.data_ptr(), c_allow, d_ids.data_ptr(), d_len.data_ptr(), d_fin.data_ptr(), _cabi.ptr(d_logits),
                                             state.data_ptr(), state.numel(), max_len, _cabi.current_stream_handle(dev), self._status.data_ptr()),
                        "at_gpt_generate")

        with self._truncated(*truncation):
            ids, _, fin, logits = self._run(call, host, uniforms, B, max_new, return_logits and B >= 1 and max_new >= 1,
                                            "at_gpt_generate: a prompt id lies outside the model's vocabulary")
        return ids, [FINISH[f] for f in fin], logits

    @contextlib.contextmanager
    def _truncated(self, top_p: float, min_p: float):
        """The handle's truncation (``at_gpt_set_truncation``) is ``(top_p, min_p)`` inside the block and off after it, also when the block raises."""
        _cabi.check(self._fn("set_truncation")(self.handle, float(top_p), float(min_p)), "at_gpt_set_truncation")
        try:
            yield
        finally:
            _cabi.check(self._fn("set_truncation")(self.handle, 1.0, 0.0), "at_gpt_set_truncation")

    def _run(self, call, host, uniforms, B, cap, return_logits, bad_id):
        """One library call around its buffers: uploads ``host`` (int32 ids) and ``uniforms``, allocates ``ids [B, cap]`` (-1), the lengths, the finish flags
        and (``return_logits``) ``logits [B, cap, V]``, runs ``call(dev, d_host, d_u, d_ids, d_len, d_fin, d_logits)``, reads back. Returns per row the ids,
        the count, the finish code and the logits ``[n + stopped, V]`` (or None); ``last_raw_ids`` keeps the whole id buffer. Status bit 0 raises ``bad_id``."""
        dev = self.device
        with torch.cuda.device(dev):
            d_host = torch.from_numpy(host).to(dev)
            d_u = torch.from_numpy(uniforms).to(dev)
            d_ids = torch.full((max(B, 1), max(cap, 1)), -1, dtype=torch.int32, device=dev)
            d_len = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
            d_fin = torch.zeros(max(B, 1), dtype=torch.int32, device=dev)
            d_logits = torch.empty((B, cap, self.vocab), dtype=torch.float32, device=dev) if return_logits else None
            call(dev, d_host, d_u, d_ids, d_len, d_fin, d_logits)
            n = d_len.cpu().tolist()    # synchronises
            fin = d_fin.cpu().tolist()
            ids_all = d_ids.cpu().to(torch.int64)
        if self.last_status() & 1:
            raise ValueError(bad_id)
        if self.last_status() & 2:
            raise ValueError("a voice prompt's code lies outside its code book")
        self.last_raw_ids = ids_all   # the whole [B, cap] buffer, -1 where nothing was written (tests)
        ids = [ids_all[b, :n[b]].clone() for b in range(B)]
        logits = None
        if d_logits is not None:
            logits = [d_logits[b, :min(cap, n[b] + (1 if fin[b] == 1 else 0))].cpu() for b in range(B)]
        return ids, n, fin, logits

    def to_acoustic(self, tokens, max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100, seed: int = 0,
                    uniforms: Optional[np.ndarray] = None, constrain: bool = False, return_logits: bool = False, top_p: Optional[float] = None,
                    min_p: Optional[float] = None) -> AcousticGeneration:
        cfg = self.config
        batch = tokens if isinstance(tokens, (list, tuple)) else [tokens]
        prompts = [prepare_source(t, cfg) for t in batch]
        allow = constrained_allow(cfg) if constrain else None   # step s: the code book of its parity, and STOP where a whole frame has been written
        ids, finish, logits = self.generate(prompts, max_new_tokens, temperature, top_k, cfg.STOP_TOKEN, uniforms, seed, allow, return_logits, top_p, min_p)
        return self._generation(ids, finish, logits)

    def _generation(self, ids, finish, logits, windows=None) -> AcousticGeneration:
        cfg = self.config
        ids = [i - cfg.ACOUSTIC_OFFSET for i in ids]
        codes: List[Optional[torch.Tensor]] = []
        for i in ids:
            try:
                codes.append(coarse_codes(i, cfg.codebook_size, cfg.num_codebooks))
            except ValueError:
                codes.append(None)
        return AcousticGeneration(ids=ids, codes=codes, finish=finish, logits=logits, windows=windows)

    def to_acoustic_long(self, tokens, window: Optional[int] = None, hop: Optional[int] = None, max_new_tokens: int = 1024, temperature: float = 0.8,
                         top_k: int = 100, seed: int = 0, uniforms: Optional[np.ndarray] = None, return_logits: bool = False,
                         slots: Optional[int] = None, tick_tokens: Optional[int] = None, voice=None, top_p: Optional[float] = None,
                         min_p: Optional[float] = None) -> AcousticGeneration:
        """``to_acoustic(constrain=True)`` for sources of any length up to 65536 ids: the source is walked in windows of ``window`` ids every
        ``hop`` ids (defaults: ``default_window``), each window prompted with the acoustic ids the window before produced for their overlap, all windows of up
        to 64 sources enqueued by one library call. Every window but a source's last produces exactly ``ids_per_source_token`` ids per source id and cannot
        stop; the last ends as ``to_acoustic`` does, within ``max_new_tokens``. ``uniforms``: float32 ``[B, L]``, the draw of a row's stream position (one per
        id of the result), ``L`` at least the longest row's capacity; from ``seed``: ``seeded_uniforms(seed, B, max(max_new_tokens, capacity))``. A source of
        at most ``window`` ids gives what ``to_acoustic(constrain=True)`` gives. ``windows`` of the result is the schedule with the counts produced.
        ``slots`` (1 to 64) runs the sources through the generation queue instead: 1 to 4096 of them share ``slots`` cache rows, each starts
        when a row is free and finishes on its own, and every source's result follows the same rule with the same draws, whatever its neighbours are.
        ``tick_tokens``: the most tokens one model pass may hold (at least ``slots`` + the longest window; default ``slots + 2`` windows). The result then
        carries ``ticks`` and ``placement`` (``queue_ticks``).
        ``voice``: a ``VoicePrompt`` that every source continues, or a list with one (or None) per source. Such a source follows the schedule
        of the prompt's ids followed by its own, its first window carrying the prompt's coarse codes as if the row had produced them; ``ids``, ``codes``,
        ``logits`` and ``uniforms`` cover what was generated only, position 0 the first id after the prompt, while ``windows`` is the schedule of the
        concatenated source. Prompts that are one object share one entry of the device's table.
        ``top_p`` / ``min_p``: the nucleus and the min-p cut after the top-k, at every step of every window; None: off."""
        cfg = self.config
        truncation = check_truncation(top_p, min_p)
        r, block = int(cfg.ids_per_source_token), self.block_size
        S = default_window(cfg, block)[0] if window is None else int(window)
        H = (S // 2) // 2 * 2 if hop is None else int(hop)
        batch = tokens if isinstance(tokens, (list, tuple)) else [tokens]
        B = len(batch)
        if slots is None:
            if tick_tokens is not None:
                raise ValueError("to_acoustic: tick_tokens= belongs to slots=")
            if not 1 <= B <= 64:
                raise ValueError(f"to_acoustic: 1 to 64 sources per call, got {B}")
        else:
            slots = int(slots)
            if not 1 <= slots <= MAX_SLOTS:
                raise ValueError(f"to_acoustic: slots must be 1 to {MAX_SLOTS}, got {slots}")
            if not 1 <= B <= MAX_QUEUE_SOURCES:
                raise ValueError(f"to_acoustic: 1 to {MAX_QUEUE_SOURCES} sources per queue call, got {B}")
        max_new = int(max_new_tokens)
        if not 1 <= max_new <= 1024:
            raise ValueError(f"to_acoustic: max_new_tokens must be 1 to 1024, got {max_new}")
        srcs = [source_ids(t, cfg) for t in batch]
        from .voice import voice_table
        table = voice_table(voice, B, cfg.SEMANTIC_VOCAB_SIZE, cfg.codebook_size, r)   # None, or (sem [n, p], codes [n, 2, f], lens, entry of each source)
        prompts = None if table is None else [int(table[2][e]) if e >= 0 else 0 for e in table[3]]
        # refuses a bad window / hop / length / prompt before anything is launched
        plans = [acoustic_windows(int(s.numel()), S, H, r, block, prompts[b] if prompts else 0) for b, s in enumerate(srcs)]
        lens = [int(s.numel()) for s in srcs]
        base, cap, longest = stream_extent(plans, S, r, max_new, block, prompts)
        if uniforms is None:
            uniforms = seeded_uniforms(seed, B, max(max_new, cap))
        uniforms = np.ascontiguousarray(uniforms, dtype=np.float32)
        if uniforms.ndim != 2 or uniforms.shape[0] != B or uniforms.shape[1] < cap:
            raise ValueError(f"uniforms must be float32 [{B}, L] with L >= {cap} (one draw per row and stream position), got {uniforms.shape}")
        if slots is not None:
            tick_tokens = slots + DEFAULT_TICK_WINDOWS * longest if tick_tokens is None else int(tick_tokens)
            if not slots + longest <= tick_tokens <= MAX_SLOTS * 1025:
                raise ValueError(f"to_acoustic: tick_tokens must be at least slots + the longest window ({slots} + {longest}) and at most {MAX_SLOTS * 1025}, "
                                 f"got {tick_tokens}")
        stride = max(lens)
        host = np.zeros((B, stride), dtype=np.int32)
        for b, s in enumerate(srcs):
            host[b, :lens[b]] = s.numpy()
        c_lens = (C.c_int32 * B)(*lens)
        queue = {}

        def call(dev, d_src, d_u, d_ids, d_len, d_fin, d_logits):
            # what the two entry points share: the sources, the geometry, the token space, the sampling arguments and the caller's arrays
            vt, form = (), ""
            if table is not None:   # the prompted forms take the table between the sources and the geometry
                d_sem, d_codes = torch.from_numpy(table[0]).to(dev), torch.from_numpy(table[1]).to(dev)
                n_p = len(table[2])
                vt = (d_sem.data_ptr(), table[0].shape[1], d_codes.data_ptr(), table[1].shape[2], (C.c_int32 * n_p)(*table[2]), n_p, (C.c_int32 * B)(*table[3]))
                form = "_prompted"
            head = (self.handle, d_src.data_ptr(), stride, c_lens, B, *vt, S, H, r, cfg.SEMANTIC_OFFSET, cfg.SEMANTIC_VOCAB_SIZE, cfg.INFER_TOKEN, cfg.ACOUSTIC_OFFSET,
                    cfg.codebook_size, cfg.STOP_TOKEN, max_new, float(temperature), int(top_k), d_u.data_ptr(), uniforms.shape[1], d_ids.data_ptr(), cap,
                    d_len.data_ptr(), d_fin.data_ptr(), _cabi.ptr(d_logits))
            tail = (_cabi.current_stream_handle(dev), self._status.data_ptr())
            if slots is None:   # the lockstep call: window k of every row as one batch
                nbytes = int(self._fn("long_state_bytes")(self.handle, B, longest))
                state = self._workspace(max(nbytes, 256))
                self._status.zero_()
                _cabi.check(self._fn("generate_long" + form)(*head, state.data_ptr(), state.numel(), longest, *tail), "at_gpt_generate_long" + form)
                return
            nbytes = int(self._fn("queue_state_bytes")(self.handle, slots, longest, tick_tokens))
            if nbytes == 0:
                raise ValueError(_cabi.last_error())
            state = self._workspace(nbytes)
            self._status.zero_()
            cap_ticks = min(queue_tick_bound(lens, S, H, r, block, max_new, prompts), 1 << 20)   # past a million ticks the trace loses its tail
            c_trace = (C.c_int32 * (4 * cap_ticks))()
            c_n = C.c_int32(0)
            c_place = (C.c_int32 * (3 * B))()
            _cabi.check(self._fn("generate_queue" + form)(*head, state.data_ptr(), state.numel(), longest, slots, tick_tokens, c_trace, cap_ticks,
                                                          C.byref(c_n), c_place, *tail), "at_gpt_generate_queue" + form)
            queue["ticks"] = [tuple(c_trace[4 * i:4 * i + 4]) for i in range(min(c_n.value, cap_ticks))]
            queue["placement"] = [tuple(c_place[3 * i:3 * i + 3]) for i in range(B)]

        with self._truncated(*truncation):
            ids, n, fin, logits = self._run(call, host, uniforms, B, cap, return_logits, "at_gpt_generate_long: a source id lies outside the semantic vocabulary")
        windows = [plan[:-1] + [plan[-1][:3] + (n[b] - base[b],)] for b, plan in enumerate(plans)]
        out = self._generation(ids, [FINISH[f] for f in fin], logits, windows)
        out.ticks, out.placement = queue.get("ticks"), queue.get("placement")
        return out

    def stream_pool(self, streams: int = 64, slots: int = 16, **kw):
        """Stage 1 of a stream pool: a ``semantic_pool.GptStreamPool`` on this model. Up to ``streams`` live streams, which start, push and
        finish on their own, share ``slots`` cache rows; each follows ``to_acoustic_long``'s schedule on its own source with its own draws."""
        from .semantic_pool import GptStreamPool
        return GptStreamPool(self, streams=streams, slots=slots, **kw)

    def score_rows(self, seqs: Sequence[np.ndarray], score_from: Sequence[int], temperature: float = 1.0, allow=None, rows: int = MAX_SLOTS,
                   pass_tokens: Optional[int] = None, head_rows: int = 1024, max_len: Optional[int] = None, return_logits: bool = False):
        """``at_gpt_score`` as it is (include/audiotoken_hip.h): ``seqs`` 1 to 65536 int id arrays over the model's own vocabulary, row b
        scored from position ``score_from[b]`` on. ``allow``: None or int ``[2][4]``. ``rows`` / ``pass_tokens`` / ``head_rows`` / ``max_len``: the cache
        rows and the tokens of one pass, the scored positions of one head chunk, the positions of a cache row (default: the longest row). Returns
        ``(logprob, rank, logits)``: per row float32 / int32 ``[len - score_from]`` on the CPU and (``return_logits``) float32 ``[len - score_from, V]``."""
        n = len(seqs)
        if not 1 <= n <= MAX_SCORE_ROWS or len(score_from) != n:
            raise ValueError(f"score_rows: 1 to {MAX_SCORE_ROWS} rows with one score_from each, got {n} and {len(score_from)}")
        lens = [int(len(s)) for s in seqs]
        froms = [int(f) for f in score_from]
        stride = max(lens + [2])
        max_len = max(2, min(self.block_size, stride)) if max_len is None else int(max_len)
        rows = int(rows)
        if pass_tokens is None:   # every cache row full, or the whole call when that is less
            pass_tokens = max(max_len, min(max(rows, 1) * max_len, sum(lens) - n))   # a row's last id takes no room in the list
        out_stride = max([l - f for l, f in zip(lens, froms)] + [1])
        host = np.zeros((n, stride), dtype=np.int32)
        for b, s in enumerate(seqs):
            host[b, :lens[b]] = np.asarray(s, dtype=np.int32)
        c_allow = None if allow is None else (C.c_int32 * 8)(*[int(v) for v in np.asarray(allow).reshape(8)])
        dev = self.device
        with torch.cuda.device(dev):
            nbytes = int(self._fn("score_state_bytes")(self.handle, rows, max_len, int(pass_tokens), int(head_rows)))
            if nbytes == 0:
                raise ValueError(_cabi.last_error())
            d_seq = torch.from_numpy(host).to(dev)
            d_lp = torch.full((n, out_stride), float("nan"), dtype=torch.float32, device=dev)
            d_rank = torch.full((n, out_stride), -1, dtype=torch.int32, device=dev)
            d_logits = torch.empty((n, out_stride, self.vocab), dtype=torch.float32, device=dev) if return_logits else None
            state = self._workspace(nbytes)
            self._status.zero_()
            _cabi.check(self._fn("score")(self.handle, d_seq.data_ptr(), stride, (C.c_int32 * n)(*lens), (C.c_int32 * n)(*froms), n, float(temperature),
                                          c_allow, d_lp.data_ptr(), d_rank.data_ptr(), out_stride, _cabi.ptr(d_logits), state.data_ptr(), state.numel(), rows,
                                          max_len, int(pass_tokens), int(head_rows), _cabi.current_stream_handle(dev), self._status.data_ptr()), "at_gpt_score")
            lp_all, rank_all = d_lp.cpu(), d_rank.cpu()   # synchronises
        if self.last_status() & 1:
            raise ValueError("at_gpt_score: an id lies outside the model's vocabulary")
        self.last_raw_scores = (lp_all, rank_all)   # the whole [n, out_stride] buffers, NaN / -1 where nothing was written (tests)
        count = [l - f for l, f in zip(lens, froms)]
        logprob = [lp_all[b, :count[b]].clone() for b in range(n)]
        rank = [rank_all[b, :count[b]].clone() for b in range(n)]
        logits = None if d_logits is None else [d_logits[b, :count[b]].cpu() for b in range(n)]
        return logprob, rank, logits

    def score_acoustic(self, tokens, codes, temperature: float = 1.0, constrain: bool = False, include_stop: bool = True, long_form: bool = False,
                       window: Optional[int] = None, hop: Optional[int] = None, return_logits: bool = False, **passes) -> AcousticScore:
        """The log-probability of given coarse codes under the model, teacher-forced (``AudioToken.score_acoustic``). ``passes``: ``rows``,
        ``pass_tokens`` and ``head_rows`` of ``score_rows``."""
        cfg = self.config
        batch = tokens if isinstance(tokens, (list, tuple)) else [tokens]
        code_list = codes if isinstance(codes, (list, tuple)) else [codes]
        if not 1 <= len(batch) <= MAX_SCORE_SOURCES:
            raise ValueError(f"score_acoustic: 1 to {MAX_SCORE_SOURCES} sources per call, got {len(batch)}")
        if len(code_list) != len(batch):
            raise ValueError(f"score_acoustic: {len(batch)} sources with {len(code_list)} code arrays")
        if not long_form and (window is not None or hop is not None):
            raise ValueError("score_acoustic: window= and hop= belong to long_form=True")
        streams = [acoustic_stream(c, cfg) for c in code_list]
        block = self.block_size
        seqs, froms, owner, place, windows = [], [], [], [], None
        if long_form:   # every window of every source is a row of one call: given the codes, the windows do not depend on each other
            S = default_window(cfg, block)[0] if window is None else int(window)
            H = (S // 2) // 2 * 2 if hop is None else int(hop)
            windows = []
            for b, (t, s) in enumerate(zip(batch, streams)):
                rows_b, plan = long_score_rows(t, s, S, H, cfg, block, include_stop)
                windows.append(plan)
                for seq, score_from, base in rows_b:
                    seqs.append(seq); froms.append(score_from); owner.append(b); place.append(base)
            if len(seqs) > MAX_SCORE_ROWS:
                raise ValueError(f"score_acoustic: the sources have {len(seqs)} windows, one call takes {MAX_SCORE_ROWS}")
        else:
            for b, (t, s) in enumerate(zip(batch, streams)):
                seq, score_from = score_row(t, s, cfg, block, include_stop)
                seqs.append(seq); froms.append(score_from); owner.append(b); place.append(0)
        allow = constrained_allow(cfg) if constrain or long_form else None
        lp, rank, logits = self.score_rows(seqs, froms, temperature, allow, return_logits=return_logits, **passes) if seqs else ([], [], [] if return_logits else None)
        out_lp, out_rank, out_logits = [], [], []
        for b, s in enumerate(streams):
            n = s.size + (1 if include_stop else 0)
            mine = [i for i, o in enumerate(owner) if o == b]   # in stream order, and they tile [0, n)
            assert sum(len(lp[i]) for i in mine) == n and all(place[i] == sum(len(lp[j]) for j in mine[:q]) for q, i in enumerate(mine))
            out_lp.append(torch.cat([lp[i] for i in mine]) if mine else torch.empty(0))
            out_rank.append(torch.cat([rank[i] for i in mine]) if mine else torch.empty(0, dtype=torch.int32))
            if return_logits:
                out_logits.append(torch.cat([logits[i] for i in mine]) if mine else torch.empty(0, self.vocab))
        nll = [float(-(x.to(torch.float64)).mean()) if x.numel() else float("nan") for x in out_lp]
        return AcousticScore(logprob=out_lp, rank=out_rank, nll=nll, windows=windows, logits=out_logits if return_logits else None)


def score_logits(logits: torch.Tensor, targets: torch.Tensor, temperature: float = 1.0, allow=None):
    """``at_op_score_rows`` on device tensors: logits float32 ``[R, V]``, targets int32 ``[R]`` -> (logprob float32 ``[R]``, rank int32 ``[R]``): the
    scoring rule alone."""
    lib = _cabi.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    assert targets.is_cuda and targets.dtype == torch.int32 and targets.is_contiguous() and targets.numel() == logits.shape[0]
    logprob = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
    rank = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    c_allow = None if allow is None else (C.c_int32 * 4)(*[int(v) for v in allow])
    with torch.cuda.device(logits.device):
        _cabi.check(lib.at_op_score_rows(logits.data_ptr(), logits.shape[0], logits.shape[1], targets.data_ptr(), float(temperature), c_allow, logprob.data_ptr(),
                                         rank.data_ptr(), _cabi.current_stream_handle(logits.device)), "at_op_score_rows")
    return logprob, rank


def topk_sample(logits: torch.Tensor, temperature: float, top_k: int, uniforms: torch.Tensor, allow=None) -> torch.Tensor:
    """``at_op_topk_sample`` on device tensors: logits float32 ``[B, V]``, uniforms float32 ``[B]`` -> int32 ``[B]`` (the sampling rule alone)."""
    lib = _cabi.load()
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    assert uniforms.is_cuda and uniforms.dtype == torch.float32 and uniforms.is_contiguous() and uniforms.numel() == logits.shape[0]
    out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    c_allow = None if allow is None else (C.c_int32 * 4)(*[int(v) for v in allow])
    with torch.cuda.device(logits.device):
        _cabi.check(lib.at_op_topk_sample(logits.data_ptr(), logits.shape[0], logits.shape[1], float(temperature), int(top_k), uniforms.data_ptr(), c_allow,
                                          out.data_ptr(), _cabi.current_stream_handle(logits.device)), "at_op_topk_sample")
    return out


def nucleus_sample(logits: torch.Tensor, temperature: float, top_k: int, uniforms: torch.Tensor, top_p: Optional[float] = None, min_p: Optional[float] = None,
                   allow=None):
    """``at_op_nucleus_sample`` on device tensors: ``topk_sample``'s arguments with the nucleus and the min-p cut (None: off) ->
    ``(token, kept, thresh)``, int32 / int32 / float32 ``[B]``: the draw, the size of the final set and its lowest tempered value."""
    lib = _cabi.load()
    p, q = check_truncation(top_p, min_p)
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    assert uniforms.is_cuda and uniforms.dtype == torch.float32 and uniforms.is_contiguous() and uniforms.numel() == logits.shape[0]
    out = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    kept = torch.empty(logits.shape[0], dtype=torch.int32, device=logits.device)
    thresh = torch.empty(logits.shape[0], dtype=torch.float32, device=logits.device)
    c_allow = None if allow is None else (C.c_int32 * 4)(*[int(v) for v in allow])
    with torch.cuda.device(logits.device):
        _cabi.check(lib.at_op_nucleus_sample(logits.data_ptr(), logits.shape[0], logits.shape[1], float(temperature), int(top_k), p, q, uniforms.data_ptr(),
                                             c_allow, out.data_ptr(), kept.data_ptr(), thresh.data_ptr(), _cabi.current_stream_handle(logits.device)),
                    "at_op_nucleus_sample")
    return out, kept, thresh
