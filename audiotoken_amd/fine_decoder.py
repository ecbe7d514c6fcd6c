"""The two coarse EnCodec code books -> all eight: stage 2 of the reference's semantic decoders (bark's ``generate_fine``, ``decoder.py:109-121`` and
``241-243``) on the HIP fine transformer (csrc/fine.hip). The loop is ``BarkFineModel.generate``: windows of ``W`` frames hopping by
``W / 2``, six forwards per window (code books 2 to 7), each writing one id per predicted position. ``history=`` is its
``history_prompt["fine_prompt"]``: the last ``W / 2`` frames of a clip's 8 code books in front of the row, read and never written.

Stated deviations from the reference: the draws come from a caller-visible uniform stream, not ``torch.multinomial``; temperature 1.0
samples (HF takes the argmax there; here only ``temperature=None`` does)."""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass
from typing import Dict, List, Optional, Union

import numpy as np
import torch

from . import _cabi
from ._handle import LibHandle
from .configs import FineDecoderConfig

N_PASSES = 6   # code books 2 to 7


@dataclass
class FineGeneration:
    """What ``to_fine`` returns, one entry per row of the batch."""
    codes: List[torch.Tensor]                          # int64 [8, T_b]: rows 0 and 1 are the input
    logits: Optional[List[torch.Tensor]] = None        # return_logits: float32 [n_b, 6, W, 1024]; positions below a window's ``rel`` hold NaN
    window_ids: Optional[List[torch.Tensor]] = None    # return_logits: int64 [n_b, 6, W], what each pass wrote (-1 below ``rel``), overwritten ones included
    passes: Optional[List[tuple]] = None               # the window queue: per pass (windows, rows admitted, rows retired), as the library ran them
    placement: Optional[List[tuple]] = None            # the window queue: per row (slot, first pass, last pass)


def fine_windows(T: int, W: int, h: int = 0):
    """The windows of a row of ``T`` frames at block ``W`` after ``h`` history cells (``history_cells``; the twin of csrc/fine.h ``fine_windows`` and
    ``fine_window``): a list of ``(start, fill)``; window ``k`` reads cells ``[start, start + W)`` of the row's work array of ``max(h + T, W)`` cells and
    predicts from ``fill`` on (buffer positions ``>= fill - start``). The row's own frames are cells ``[h, h + T)``."""
    H, L = W // 2, max(h + T, W)
    n = max(0, -(-(h + T - W) // H)) + 1
    return [(min(k * H, L - W), min(h + k * H, L - H)) for k in range(n)]


def history_cells(Th: int, W: int) -> int:
    """The cells a history of ``Th`` frames takes in front of a row: its last ``min(W / 2, Th)`` frames."""
    return min(W // 2, Th)


def seeded_uniforms(seed: int, batch: int, n_max: int, block: int) -> np.ndarray:
    return np.random.Generator(np.random.Philox(seed)).random((batch, n_max, N_PASSES, block), dtype=np.float32)


def row_uniforms(seed: int, row: int, n_windows: int, block: int) -> np.ndarray:
    """The queue's draws of row ``row`` from ``seed``: float32 ``[n_windows, 6, block]`` from a Philox stream keyed by (seed, row), so that a row's draws
    do not depend on the other rows' lengths."""
    return np.random.Generator(np.random.Philox(key=[seed, row])).random((n_windows, N_PASSES, block), dtype=np.float32)


MAX_QUEUE_ROWS, MAX_SLOTS = 4096, 64


def fine_queue_passes(lens, W: int, slots: int):
    """The window queue's schedule (the twin of csrc/fine.h ``FineQueueSchedule``) for rows of ``lens`` frames through ``slots`` work
    arrays: ``(passes, placement)``. ``passes[p]`` lists the ``(slot, row, k)`` of every window of pass p in slot order; ``placement[b]`` is row b's
    ``(slot, first pass, last pass)``. Rows take empty slots in order; a slot runs its row's windows in consecutive passes and takes the next waiting row
    in the pass after its row's last window."""
    lens = [int(T) for T in lens]
    if not 1 <= slots <= MAX_SLOTS:
        raise ValueError(f"slots must be 1 to {MAX_SLOTS}, got {slots}")
    if not 1 <= len(lens) <= MAX_QUEUE_ROWS:
        raise ValueError(f"1 to {MAX_QUEUE_ROWS} rows per call, got {len(lens)}")
    if min(lens) < 1:
        raise ValueError("every row needs at least one frame")
    n = [len(fine_windows(T, W)) for T in lens]
    holds, at = [None] * slots, [0] * slots
    waiting, passes, placement = 0, [], [None] * len(lens)
    while True:
        this = []
        for j in range(slots):
            if holds[j] is None and waiting < len(lens):
                holds[j], at[j] = waiting, 0
                placement[waiting] = (j, len(passes), None)
                waiting += 1
            if holds[j] is None:
                continue
            b = holds[j]
            this.append((j, b, at[j]))
            at[j] += 1
            if at[j] == n[b]:
                placement[b] = (placement[b][0], placement[b][1], len(passes))
                holds[j] = None
        if not this:
            return passes, placement
        passes.append(this)


def _shape_and_kind(x):
    if isinstance(x, torch.Tensor):   # no copy off the device for a look at its shape
        return tuple(x.shape), "f" if (x.dtype.is_floating_point or x.dtype.is_complex) else "b" if x.dtype == torch.bool else "i"
    a = np.asarray(x)
    return a.shape, a.dtype.kind


def _as_histories(history, n_rows: int, W: int, check_only: bool = False):
    """``history=`` of a call: None, one ``[8, Th]`` array shared by every row, or a list with one array (or None) per row. Returns the table (distinct
    arrays, int32 ``[8, min(Th, W / 2)]``: only the last ``W / 2`` frames are ever read, so only they are kept and uploaded), the table entry of each row
    (-1 for none) and the history cells ``h`` of each row. One OBJECT is one table entry however many rows name it; equal arrays that are distinct
    objects are distinct entries. ``check_only``: the refusals alone, from shapes and dtypes, nothing converted or copied (returns None)."""
    if history is None:
        return [], [-1] * n_rows, [0] * n_rows
    per_row = list(history) if isinstance(history, (list, tuple)) else [history] * n_rows
    if len(per_row) != n_rows:
        raise ValueError(f"to_fine: history must be None, one [8, Th] array or a list of {n_rows} (one per row), got a list of {len(per_row)}")
    table, entry_of, of_row = [], {}, []
    for i, hst in enumerate(per_row):
        if hst is None:
            of_row.append(-1)
            continue
        if id(hst) not in entry_of:
            shape, kind = _shape_and_kind(hst)
            if len(shape) != 2 or shape[0] != 8 or shape[1] < 1 or kind not in "iu":
                raise ValueError(f"to_fine: the history of row {i} must be integer codes [8, Th] with Th >= 1, got {getattr(hst, 'dtype', kind)} {tuple(shape)}")
            if shape[1] > MAX_HISTORY:
                raise ValueError(f"to_fine: a history holds at most {MAX_HISTORY} frames, got {shape[1]}")
            entry_of[id(hst)] = len(table)
            if check_only:
                table.append(None)
            else:
                last = hst[:, -(W // 2):] if W >= 2 else hst   # the frames a window can read
                a = np.asarray(last.cpu() if isinstance(last, torch.Tensor) else last)
                table.append(np.clip(a.astype(np.int64), -1, 1024).astype(np.int32))   # what lies outside stays outside after the narrowing
        of_row.append(entry_of[id(hst)])
    if check_only:
        return None
    return table, of_row, [0 if e < 0 else history_cells(table[e].shape[1], W) for e in of_row]


MAX_HISTORY = 1 << 18


def _as_rows(codes) -> List[np.ndarray]:
    batch = list(codes) if isinstance(codes, (list, tuple)) else [codes]
    rows = []
    for i, c in enumerate(batch):
        a = np.asarray(c.cpu() if isinstance(c, torch.Tensor) else c)
        if a.ndim == 3 and a.shape[0] == 1:
            a = a[0]
        if a.ndim != 2 or a.shape[0] != 2 or a.shape[1] < 1 or a.dtype.kind not in "iu":
            raise ValueError(f"to_fine: row {i} must be integer coarse codes [2, T] with T >= 1, got {a.dtype} {tuple(a.shape)}")
        rows.append(np.ascontiguousarray(a, dtype=np.int64))
    return rows


class _HistoryTable:
    """What a call passes for its history table; the empty table by default."""
    dev = lens = of_row = None
    max_hist = 0
    args = ()


class CoarseToFine(LibHandle):
    """Owner of one ``at_fine`` handle. ``weights``: a checkpoint path, a ``{name: array}`` dict, or None for the seeded synthetic model."""

    FAMILY = "fine"

    def __init__(self, config: Optional[FineDecoderConfig] = None, device="cuda:0", weights: Union[None, str, os.PathLike, Dict[str, np.ndarray]] = None):
        self.config = config or FineDecoderConfig()
        if weights is None:
            weights = self.config.weights

        def host_tensors():
            from . import weights as W
            if weights is None:
                return W.synth_fine_weights(self.config.synthetic_layers, self.config.synthetic_hidden, self.config.synthetic_block)
            if isinstance(weights, dict):
                return W.fine_tensors_from_state_dict(weights, "weights dict")
            return W.read_fine_checkpoint(weights)

        self._create(device, None, host_tensors)

    def _finish_init(self) -> None:
        self.n_layers = self._fn("num_layers")(self.handle)
        self.hidden = self._fn("hidden")(self.handle)
        self.block_size = self._fn("block_size")(self.handle)
        self.has_bias = bool(self._fn("has_bias")(self.handle))
        self._init_call_state()

    def eval(self):
        return self

    def generate(self, codes, temperature: Optional[float] = 0.5, seed: int = 0, uniforms: Optional[np.ndarray] = None,
                 return_logits: bool = False, history=None) -> FineGeneration:
        """``codes``: integer ``[2, T]`` or a list of 1 to 64 of them, each of its own length. ``temperature=None``: the argmax, the lowest id among
        equals. ``uniforms``: float32 ``[B, n_max, 6, W]``, the draw of row b, window k, code book 2 + j and buffer position t (``n_max``: the windows
        of the longest row); from ``seed`` otherwise (``seeded_uniforms``). ``history``: None, integer ``[8, Th]`` codes that every row continues, or a
        list with one such array (or None) per row; a row's windows are then ``fine_windows(T, W, history_cells(Th, W))`` and the result
        holds the row's own frames only."""
        rows = _as_rows(codes)
        B, W = len(rows), self.block_size
        if not 1 <= B <= self.config.max_rows:
            raise ValueError(f"to_fine: 1 to {self.config.max_rows} rows per call, got {B}")
        lens = [int(r.shape[1]) for r in rows]
        table, of_row, hcells = _as_histories(history, B, W)
        n = [len(fine_windows(T, W, h)) for T, h in zip(lens, hcells)]
        n_max, max_T = max(n), max(lens)
        greedy = temperature is None
        if not greedy:
            if uniforms is None:
                uniforms = seeded_uniforms(seed, B, n_max, W)
            uniforms = np.ascontiguousarray(uniforms, dtype=np.float32)
            if uniforms.shape != (B, n_max, N_PASSES, W):
                raise ValueError(f"uniforms must be float32 [{B}, {n_max}, {N_PASSES}, {W}] (row, window, code book, buffer position), got {uniforms.shape}")
        host = np.zeros((B, 2, max_T), dtype=np.int32)
        for b, r in enumerate(rows):
            host[b, :, :lens[b]] = np.clip(np.asarray(r).astype(np.int64), -1, self.config.codebook_size)   # what lies outside stays outside after the narrowing
        dev = self.device
        with torch.cuda.device(dev):
            d_codes = torch.from_numpy(host).to(dev)
            d_u = None if greedy else torch.from_numpy(uniforms).to(dev)
            d_out = torch.full((B, 8, max_T), -1, dtype=torch.int32, device=dev)
            d_logits = d_ids = None
            if return_logits:
                d_logits = torch.full((B, n_max, N_PASSES, W, 1024), float("nan"), dtype=torch.float32, device=dev)
                d_ids = torch.full((B, n_max, N_PASSES, W), -1, dtype=torch.int32, device=dev)
            hist = self._history_table(table, of_row)
            nbytes = int(self._fn("state_bytes_hist")(self.handle, B, max_T, hist.max_hist) if table else self._fn("state_bytes")(self.handle, B, max_T))
            if nbytes == 0:
                raise _cabi.HipLibraryError(f"at_fine_state_bytes failed: {_cabi.last_error()}")
            state = self._workspace(nbytes)
            self._status.zero_()
            c_lens = (C.c_int32 * B)(*lens)
            tail = (1.0 if greedy else float(temperature), 1 if greedy else 0, _cabi.ptr(d_u), n_max, d_out.data_ptr(), _cabi.ptr(d_logits), _cabi.ptr(d_ids),
                    state.data_ptr(), state.numel(), max_T, _cabi.current_stream_handle(dev), self._status.data_ptr())
            if table:
                _cabi.check(self._fn("generate_hist")(self.handle, d_codes.data_ptr(), max_T, c_lens, B, *hist.args, *tail), "at_fine_generate_hist")
            else:
                _cabi.check(self._fn("generate")(self.handle, d_codes.data_ptr(), max_T, c_lens, B, *tail), "at_fine_generate")
            out = d_out.cpu().to(torch.int64)   # synchronises
        self._raise_status("at_fine_generate")
        self.last_raw_codes = out   # the whole [B, 8, max_T] buffer, -1 where nothing was written (tests)
        result = FineGeneration(codes=[out[b, :, :lens[b]].clone() for b in range(B)])
        if return_logits:
            result.logits = [d_logits[b, :n[b]].cpu() for b in range(B)]
            result.window_ids = [d_ids[b, :n[b]].cpu().to(torch.int64) for b in range(B)]
        return result

    def _history_table(self, table, of_row):
        """The history table of a call on the device (``[n_hist][8][h_stride]``) and the arguments that describe it, in the C ABI's order."""
        hist = _HistoryTable()
        if table:
            hist.max_hist = max(a.shape[1] for a in table)
            host = np.zeros((len(table), 8, hist.max_hist), dtype=np.int32)
            for i, a in enumerate(table):
                host[i, :, :a.shape[1]] = a
            hist.dev = torch.from_numpy(host).to(self.device)
            hist.lens = (C.c_int32 * len(table))(*[a.shape[1] for a in table])
            hist.of_row = (C.c_int32 * len(of_row))(*of_row)
            hist.args = (hist.dev.data_ptr(), hist.max_hist, hist.lens, len(table), hist.of_row, hist.max_hist)
        return hist

    def _raise_status(self, who: str) -> None:
        status = self.last_status()
        if status & 1:
            raise ValueError(f"{who}: a coarse code lies outside [0, 1024)")
        if status & 2:
            raise ValueError(f"{who}: a history id lies outside [0, 1024)")

    def generate_queue(self, codes, slots: int = 64, temperature: Optional[float] = 0.5, seed: int = 0, uniforms: Optional[List[np.ndarray]] = None,
                       return_logits: bool = False, history=None) -> FineGeneration:
        """The window queue: 1 to 4096 rows through ``slots`` (1 to 64) work arrays, each row starting when a slot is free and leaving
        after its last window; a pass batches the current window of every occupied slot, whatever its ``k``. A row's result is what ``generate`` gives
        on the row alone with the same draws. ``uniforms``: a list of per-row float32 ``[n_b, 6, W]``; from ``seed`` row b draws ``row_uniforms(seed, b,
        n_b, W)``, which does not depend on the other rows. The result also carries ``passes`` and ``placement`` as the library ran them. ``history``: as
        in ``generate``; one shared array is one table entry on the device however many rows continue it."""
        rows = _as_rows(codes)
        n_rows, W = len(rows), self.block_size
        if not 1 <= n_rows <= MAX_QUEUE_ROWS:
            raise ValueError(f"to_fine: 1 to {MAX_QUEUE_ROWS} rows per call with slots=, got {n_rows}")
        if not (isinstance(slots, (int, np.integer)) and 1 <= slots <= MAX_SLOTS):
            raise ValueError(f"to_fine: slots must be 1 to {MAX_SLOTS}, got {slots!r}")
        slots = int(slots)
        lens = [int(r.shape[1]) for r in rows]
        table, of_row, hcells = _as_histories(history, n_rows, W)
        n = [len(fine_windows(T, W, h)) for T, h in zip(lens, hcells)]
        max_T, cells = max(lens), sum(n)
        greedy = temperature is None
        flat_u = None
        if not greedy:
            if uniforms is None:
                uniforms = [row_uniforms(seed, b, n[b], W) for b in range(n_rows)]
            if not isinstance(uniforms, (list, tuple)) or len(uniforms) != n_rows:
                raise ValueError(f"uniforms must be a list of {n_rows} float32 arrays [n_b, {N_PASSES}, {W}], one per row")
            for b, u in enumerate(uniforms):
                if np.shape(u) != (n[b], N_PASSES, W):
                    raise ValueError(f"uniforms[{b}] must be float32 [{n[b]}, {N_PASSES}, {W}] (window, code book, buffer position), got {np.shape(u)}")
            flat_u = np.concatenate([np.asarray(u, dtype=np.float32).reshape(-1) for u in uniforms])
        off = np.concatenate([[0], np.cumsum(lens)])
        woff = np.concatenate([[0], np.cumsum(n)])
        host = np.concatenate([np.clip(np.asarray(r).astype(np.int64), -1, self.config.codebook_size).astype(np.int32).reshape(-1) for r in rows])   # row b: [2][T_b] at 2 off[b]
        dev = self.device
        with torch.cuda.device(dev):
            d_codes = torch.from_numpy(host).to(dev)
            d_u = None if greedy else torch.from_numpy(flat_u).to(dev)
            d_out = torch.full((8 * int(off[-1]),), -1, dtype=torch.int32, device=dev)
            d_logits = d_ids = None
            if return_logits:
                d_logits = torch.full((cells, N_PASSES, W, 1024), float("nan"), dtype=torch.float32, device=dev)
                d_ids = torch.full((cells, N_PASSES, W), -1, dtype=torch.int32, device=dev)
            hist = self._history_table(table, of_row)
            nbytes = int(self._fn("queue_state_bytes_hist")(self.handle, slots, max_T, hist.max_hist) if table
                         else self._fn("queue_state_bytes")(self.handle, slots, max_T))
            if nbytes == 0:
                raise _cabi.HipLibraryError(f"at_fine_queue_state_bytes failed: {_cabi.last_error()}")
            state = self._workspace(nbytes)
            self._status.zero_()
            c_lens = (C.c_int32 * n_rows)(*lens)
            cap = cells   # a pass holds at least one window
            trace = (C.c_int32 * (3 * cap))()
            n_passes = (C.c_int32 * 1)()
            placement = (C.c_int32 * (3 * n_rows))()
            tail = (1.0 if greedy else float(temperature), 1 if greedy else 0, _cabi.ptr(d_u), d_out.data_ptr(), _cabi.ptr(d_logits), _cabi.ptr(d_ids),
                    state.data_ptr(), state.numel(), max_T, slots, trace, cap, n_passes, placement, _cabi.current_stream_handle(dev), self._status.data_ptr())
            if table:
                _cabi.check(self._fn("generate_queue_hist")(self.handle, d_codes.data_ptr(), c_lens, n_rows, *hist.args, *tail), "at_fine_generate_queue_hist")
            else:
                _cabi.check(self._fn("generate_queue")(self.handle, d_codes.data_ptr(), c_lens, n_rows, *tail), "at_fine_generate_queue")
            out = d_out.cpu().to(torch.int64)   # synchronises
        self._raise_status("at_fine_generate_queue")
        self.last_raw_codes = out   # the whole ragged buffer (tests)
        result = FineGeneration(codes=[out[8 * off[b]:8 * off[b + 1]].reshape(8, lens[b]).clone() for b in range(n_rows)])
        result.passes = [tuple(trace[3 * p:3 * p + 3]) for p in range(n_passes[0])]
        result.placement = [tuple(placement[3 * b:3 * b + 3]) for b in range(n_rows)]
        if return_logits:
            result.logits = [d_logits[woff[b]:woff[b + 1]].cpu() for b in range(n_rows)]
            result.window_ids = [d_ids[woff[b]:woff[b + 1]].cpu().to(torch.int64) for b in range(n_rows)]
        return result
