"""Stateful resampling of streamed audio (``at_resample_rows``): any chunking gives the samples of resampling the whole signal once.

The device feeder's resampling rule is evaluated at stream-global (file-global) sample positions. For a signal of ``L`` source samples, output ``j`` in
``[0, ceil(n L / o))`` is, with ``f = j // n``, ``p = j % n``, ``base = f o - width``::

    y[j] = sum over k in [lo_p, hi_p), ascending, of fmaf(K[p][k], x[base + k], acc),    x[s] = 0 for s < 0 or s >= L

(table, phases and tap ranges of ``audio_io.resample_table``). Three layers:

* the PLANNER (pure integers, ``plan_push``): per stream, which outputs a push may emit — before the end of the signal is known frame ``f`` is ready when
  ``f o + width + o <= L_avail`` — and which source samples the stream must carry over: the tail from ``F o - width`` on (``F`` = frames emitted), fewer
  than ``2 width + o`` samples. A stream opens with ``width`` stored zeros at positions ``-width .. -1``, so every tap of a push lies in its window;
* ``DeviceResampler``: rows of (window on the device, plan) -> one ``at_resample_rows`` launch into one ``[rows][max_len]`` buffer. The descriptors are
  checked on the host (``at_resample_rows_check``) before every launch. ``HostResampler`` is its stand-in where no device is involved (the host-side
  bookkeeping of the streams is tested with it, like ``push_fn``): the same rule in float64;
* ``ResidentFiles``: the ``resample="file"`` route of ``encode`` / ``encode_batch_files`` with ``stream=True``. A file's PCM goes to the device once, in its
  storage format, and stays there from its first tick to its flush; tick ``c`` is outputs ``[ceil(n c step / o), ceil(n (c + 1) step / o))`` of the file.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Callable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _cabi
from .audio_io import resample_table

DEFAULT_MAX_FILE_BYTES = 4 << 30


# ---- the planner: integers only --------------------------------------------------------------------------------------------------------------------
def ratio(orig_freq: int, new_freq: int) -> Tuple[int, int, int]:
    """``(o, n, width)`` of resampling ``orig_freq -> new_freq``; ``(1, 1, 0)`` at the native rate (no table: conversion only)."""
    if int(orig_freq) == int(new_freq):
        return 1, 1, 0
    _, _, o, n, width = resample_table(int(orig_freq), int(new_freq))
    return o, n, width


def ceil_div(a: int, b: int) -> int:
    return -(-a // b)


@dataclass
class StreamPosition:
    """Where a stream stands: ``received`` source samples so far (``L_avail``), ``frames`` whole output frames emitted (``F``: ``F n`` outputs)."""
    o: int
    n: int
    width: int
    received: int = 0
    frames: int = 0
    emitted: int = 0       # outputs emitted: frames * n until the final push
    finished: bool = False

    @property
    def tail_base(self) -> int:
        """Global index of the first source sample the stream still holds (negative while the stored zeros are part of the tail)."""
        return self.frames * self.o - self.width

    @property
    def tail_len(self) -> int:
        return self.received - self.tail_base


@dataclass(frozen=True)
class PushPlan:
    """One push of one stream, as ``at_resample_row`` needs it. The window = the carried tail followed by the new samples; ``keep`` = how many samples at
    the END of the window are the next push's tail."""
    out_start: int
    out_len: int
    src_base: int
    src_len: int
    src_total: int
    final: bool
    keep: int
    frames_after: int

    def row(self, pcm_ptr: int, table_ptr: int, fmt: int, scale: float, o: int, n: int, width: int, dst_off: int) -> tuple:
        """The fields of ``_cabi.ResampleRow`` in order."""
        return (pcm_ptr, table_ptr, self.src_base, self.src_len, self.src_total, self.out_start, self.out_len, fmt, float(scale), o, n, width,
                1 if self.final else 0, 0, dst_off)


def plan_push(pos: StreamPosition, n_new: int, final: bool) -> PushPlan:
    """What a stream at ``pos`` emits and keeps when ``n_new`` more source samples arrive (``final``: they are the last). Pure: ``pos`` is not changed."""
    assert not pos.finished, "push after the final one"
    assert n_new >= 0
    o, n, width = pos.o, pos.n, pos.width
    L = pos.received + n_new
    if final:
        frames_after = ceil_div(L, o)     # every frame that holds an output
        out_end = ceil_div(n * L, o)
    else:
        frames_after = max(pos.frames, (L - width) // o) if L >= width else pos.frames
        out_end = frames_after * n
    keep = 0 if final else L - (frames_after * o - width)
    return PushPlan(out_start=pos.emitted, out_len=out_end - pos.emitted, src_base=pos.tail_base, src_len=pos.tail_len + n_new, src_total=L if final else 0,
                    final=bool(final), keep=keep, frames_after=frames_after)


def commit(pos: StreamPosition, plan: PushPlan) -> None:
    pos.received = plan.src_base + plan.src_len
    pos.frames = plan.frames_after
    pos.emitted = plan.out_start + plan.out_len
    pos.finished = plan.final


def file_tick_plan(L: int, o: int, n: int, step: int, c: int) -> PushPlan:
    """Tick ``c`` of a resident file of ``L`` source samples cut every ``step`` of them: outputs ``[ceil(n c step / o), ceil(n (c + 1) step / o))``
    clipped to the file. The window is the whole file, so every row is final."""
    total = ceil_div(n * L, o)
    a = min(total, ceil_div(n * c * step, o))
    b = min(total, ceil_div(n * (c + 1) * step, o))
    return PushPlan(out_start=a, out_len=b - a, src_base=0, src_len=L, src_total=L, final=True, keep=0, frames_after=0)


# ---- the rule in float64 on the host ------------------------------------------------------------------------------------------------------------------
def evaluate_plan(window: np.ndarray, plan: PushPlan, rate: int, model_rate: int) -> np.ndarray:
    """float64 evaluation of one row: ``window`` = the row's source samples as floats (already converted), positions as in ``plan``; the float32 table,
    every tap k in [0, 2 width + o) in ascending order (a zero weight adds an exact zero). Chunked or whole, every output sees the same sum."""
    window = np.asarray(window, dtype=np.float64)
    assert window.shape == (plan.src_len,)
    j = np.arange(plan.out_start, plan.out_start + plan.out_len, dtype=np.int64)
    lo_valid = max(plan.src_base, 0)
    hi_valid = plan.src_base + plan.src_len
    if plan.final:
        hi_valid = min(hi_valid, plan.src_total)
    if int(rate) == int(model_rate):
        ok = (j >= lo_valid) & (j < hi_valid)
        return np.where(ok, window[np.clip(j - plan.src_base, 0, max(plan.src_len - 1, 0))] if plan.src_len else 0.0, 0.0)
    kernels, _, o, n, width = resample_table(int(rate), int(model_rate))
    K = kernels[:, 0].numpy().astype(np.float64)
    f, p = j // n, j % n
    base = f * o - width
    acc = np.zeros(len(j), dtype=np.float64)
    for k in range(2 * width + o):
        s = base + k
        ok = (s >= lo_valid) & (s < hi_valid)
        x = np.where(ok, window[np.clip(s - plan.src_base, 0, max(plan.src_len - 1, 0))] if plan.src_len else 0.0, 0.0)
        acc = acc + K[p, k] * x
    return acc


# ---- input samples ---------------------------------------------------------------------------------------------------------------------------------
_TORCH_FMT = {torch.int16: (_cabi.PCM_S16, 1.0 / 32768.0), torch.float32: (_cabi.PCM_F32, 1.0)}


def as_pcm(samples, device=None) -> torch.Tensor:
    """Raw samples of a push — torch or numpy, float32 or int16 — as a tensor (on ``device`` when given), in their own format."""
    if isinstance(samples, np.ndarray):
        samples = torch.from_numpy(np.ascontiguousarray(samples))
    if not isinstance(samples, torch.Tensor) or samples.dtype not in _TORCH_FMT:
        raise TypeError(f"samples at a stream's own rate must be float32 or int16 (torch or numpy), not {getattr(samples, 'dtype', type(samples))}")
    return samples.to(device) if device is not None else samples


def to_float(pcm: torch.Tensor) -> torch.Tensor:
    return pcm.to(torch.float32) * (1.0 / 32768.0) if pcm.dtype == torch.int16 else pcm


# ---- the launch ------------------------------------------------------------------------------------------------------------------------------------------
class Job:
    """One row: ``pcm`` = the window (1-D, contiguous, storage format ``fmt`` / ``scale``), resampled from ``rate`` by ``plan``."""
    __slots__ = ("pcm", "fmt", "scale", "rate", "plan")

    def __init__(self, pcm: torch.Tensor, rate: int, plan: PushPlan, fmt: Optional[int] = None, scale: Optional[float] = None):
        self.pcm, self.rate, self.plan = pcm, int(rate), plan
        self.fmt, self.scale = (fmt, scale) if fmt is not None else _TORCH_FMT[pcm.dtype]


class DeviceResampler:
    """``run(jobs) -> [float32 [out_len] per job]``: views of ONE ``[rows][max_len]`` device buffer written by ONE ``at_resample_rows`` launch on the
    current stream. Rows may differ in rate, format and length."""

    def __init__(self, device, model_sample_rate: int):
        self.device = torch.device(device)
        assert self.device.type == "cuda", "the device resampler needs a HIP device"
        self.lib = _cabi.load()
        self.sr = int(model_sample_rate)
        self._tables = {}
        self.launches = 0

    def table(self, rate: int) -> Tuple[int, int, int, int]:
        """``(device pointer or 0, o, n, width)`` of ``rate -> model rate``: the blob the feeder's kernel reads ([n][kw] float32, then [n][2] int32)."""
        rate = int(rate)
        if rate == self.sr:
            return 0, 1, 1, 0
        if rate not in self._tables:
            kernels, ranges, o, n, width = resample_table(rate, self.sr)
            blob = np.concatenate([kernels[:, 0].numpy().reshape(-1).view(np.uint8), ranges.reshape(-1).view(np.uint8)])
            self._tables[rate] = (torch.from_numpy(blob).to(self.device), o, n, width)
        t, o, n, width = self._tables[rate]
        return t.data_ptr(), o, n, width

    def run(self, jobs: Sequence[Job]) -> List[torch.Tensor]:
        if not jobs:
            return []
        max_len = max(j.plan.out_len for j in jobs)
        max_len = (max_len + 3) // 4 * 4          # every row starts 16-byte aligned
        out = torch.empty((len(jobs), max_len), dtype=torch.float32, device=self.device)
        views = [out[r, :j.plan.out_len] for r, j in enumerate(jobs)]
        if max_len == 0:
            return views
        rows = (_cabi.ResampleRow * len(jobs))()
        for r, j in enumerate(jobs):
            assert j.pcm.is_cuda and j.pcm.dim() == 1 and j.pcm.is_contiguous() and j.pcm.numel() * j.pcm.element_size() >= j.plan.src_len * _ITEM[j.fmt]
            tptr, o, n, width = self.table(j.rate)
            # a window without samples still needs an address the checker accepts; it is never read (no tap is inside an empty window)
            rows[r] = _cabi.ResampleRow(*j.plan.row(j.pcm.data_ptr() or out.data_ptr(), tptr, j.fmt, j.scale, o, n, width, r * max_len))
        _cabi.check(self.lib.at_resample_rows_check(C.addressof(rows), len(jobs)), "at_resample_rows_check")
        d_rows = torch.from_numpy(np.frombuffer(rows, dtype=np.uint8).copy()).to(self.device)
        with torch.cuda.device(self.device):
            _cabi.check(self.lib.at_resample_rows(d_rows.data_ptr(), len(jobs), out.data_ptr(), _cabi.current_stream_handle(self.device)), "at_resample_rows")
        self.launches += 1
        return views


_ITEM = {_cabi.PCM_S16: 2, _cabi.PCM_S32: 4, _cabi.PCM_F32: 4, _cabi.PCM_U8: 1}


class HostResampler:
    """Stand-in for ``DeviceResampler`` where the streams run on stubs (``push_fn``): the rule in float64 on the host, rounded to float32 once."""

    def __init__(self, model_sample_rate: int):
        self.sr = int(model_sample_rate)
        self.launches = 0

    def table(self, rate: int) -> Tuple[int, int, int, int]:
        return (0,) + ratio(rate, self.sr)

    def run(self, jobs: Sequence[Job]) -> List[torch.Tensor]:
        self.launches += 1 if jobs else 0
        return [torch.from_numpy(evaluate_plan(to_float(j.pcm).numpy()[:j.plan.src_len], j.plan, j.rate, self.sr).astype(np.float32)) for j in jobs]


class RateState:
    """What a stream with a sample rate of its own carries between pushes: its position and the tail ``[B, < 2 width + o]`` in the pushes' format."""

    def __init__(self, rate: int, model_rate: int, batch: int = 1):
        self.rate, self.batch = int(rate), int(batch)
        assert self.rate >= 1, "sample_rate must be positive"
        self.ratio = ratio(self.rate, model_rate)
        self.reset()

    def reset(self) -> None:
        self.pos = StreamPosition(*self.ratio)
        self.tail: Optional[torch.Tensor] = None

    def window(self, samples: Optional[torch.Tensor], device=None) -> Tuple[torch.Tensor, int]:
        """``(tail + samples [B, t], samples per row that are new)``; ``samples`` None: nothing new (a flush)."""
        if samples is not None:
            samples = as_pcm(samples, device)
            assert samples.dim() == 2 and samples.shape[0] == self.batch, f"samples must be [{self.batch}, n]"
        if self.tail is None:     # the stream opens with `width` zeros at positions -width .. -1, in the format of its first samples
            like = samples if samples is not None else torch.empty(0, dtype=torch.float32, device=device)
            self.tail = torch.zeros((self.batch, self.pos.width), dtype=like.dtype, device=like.device)
        if samples is None:
            return self.tail, 0
        if samples.dtype != self.tail.dtype:
            raise TypeError(f"a stream keeps the sample format of its first push ({self.tail.dtype}), not {samples.dtype}")
        return torch.cat([self.tail, samples], dim=1).contiguous(), int(samples.shape[1])

    def jobs(self, window: torch.Tensor, plan: PushPlan) -> List[Job]:
        return [Job(window[b], self.rate, plan) for b in range(self.batch)]

    def advance(self, window: torch.Tensor, plan: PushPlan) -> None:
        self.tail = window[:, window.shape[1] - plan.keep:].clone() if plan.keep else window[:, :0]
        commit(self.pos, plan)


# ---- resample="file": files resident on the device ---------------------------------------------------------------------------------------------------------
@dataclass
class ResidentFile:
    name: str
    pcm: torch.Tensor      # device, the file's samples in storage format (as bytes)
    fmt: int
    scale: float
    rate: int
    length: int            # source samples
    step: int              # source samples per tick
    ratio: Tuple[int, int, int]

    @property
    def out_length(self) -> int:
        return ceil_div(self.ratio[1] * self.length, self.ratio[0])

    @property
    def ticks(self) -> int:
        return ceil_div(self.length, self.step)

    def job(self, c: int) -> Job:
        return Job(self.pcm, self.rate, file_tick_plan(self.length, self.ratio[0], self.ratio[1], self.step, c), self.fmt, self.scale)


class ResidentFiles:
    """The host side of ``resample="file"``: files (and archive members) are read ahead in their storage format by the device feeder's decoders, uploaded once
    and kept on the device while they are live; ``chunks(rows)`` is one launch for the next chunk of every live file."""

    def __init__(self, device, model_sample_rate: int, chunk_size: int, num_workers: int = 0, on_skip: Optional[Callable[[str, str], None]] = None,
                 max_file_bytes: int = DEFAULT_MAX_FILE_BYTES, min_samples: int = 0):
        from .feeder import DeviceFeeder
        self.device = torch.device(device)
        self.sr = int(model_sample_rate)
        self.chunk_size = chunk_size
        self.on_skip = on_skip or (lambda name, why: None)
        self.max_file_bytes = int(max_file_bytes)
        self.min_samples = int(min_samples)
        self.feeder = DeviceFeeder(self.device, self.sr, chunk_size, 1, 0, num_workers, self.on_skip)
        self.resampler = DeviceResampler(self.device, self.sr)

    def _open(self, name: str, raw) -> Optional[ResidentFile]:
        from .feeder import _FMT
        if raw.pcm.shape[0] != 1:
            self.on_skip(str(name), f"Audio needs to be mono, provided {raw.pcm.shape[0]} channels for {name}")
            return None
        if raw.pcm.nbytes > self.max_file_bytes:
            self.on_skip(str(name), f"{raw.pcm.nbytes} bytes of PCM exceed max_file_bytes = {self.max_file_bytes} (resample='file' keeps a file on the device)")
            return None
        length = int(raw.pcm.shape[-1])
        rt = ratio(raw.sample_rate, self.sr)
        if ceil_div(rt[1] * length, rt[0]) < self.min_samples:
            self.on_skip(str(name), f"fewer than {self.min_samples} samples")
            return None
        fmt = _FMT[raw.pcm.dtype]
        pcm = self.feeder._upload_raw(raw)                     # on the feeder's stream
        cur = torch.cuda.current_stream(self.device)
        cur.wait_stream(self.feeder.stream)                    # the resample launches of this file's ticks come after its upload
        pcm.record_stream(cur)
        step = int(self.chunk_size * raw.sample_rate)
        assert step >= 1, "chunk_size too small for this sample rate"
        return ResidentFile(str(name), pcm, fmt, float(raw.scale), int(raw.sample_rate), length, step, rt)

    def open_all(self, files: Sequence[str]) -> Iterator[ResidentFile]:
        """Every decodable mono file / archive member in order, opened (uploaded) when the consumer asks for it; decoding runs ahead on the host."""
        from .prefetch import ordered_map
        for source in ordered_map(self.feeder._decode, [str(f) for f in files], self.feeder.num_workers):
            try:
                for name, raw in source:
                    f = self._open(name, raw)
                    if f is not None:
                        yield f
            finally:
                close = getattr(source, "close", None)
                if close is not None:
                    close()

    def chunks(self, rows: Sequence[Tuple[ResidentFile, int]]) -> List[torch.Tensor]:
        """Chunk ``c`` of every ``(file, c)``: float32 views of one buffer, one launch."""
        return self.resampler.run([f.job(c) for f, c in rows])

    def finish(self) -> None:
        self.feeder._reap(wait=True)
