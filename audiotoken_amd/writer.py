"""Output side of ``decode_batch_files``: a tree of ``.npy`` token files -> a tree of 16-bit PCM WAV files, or of FLAC files
(``audio_format="flac"``: the same samples, compressed on the device by csrc/flac_encode.hip, framed on the host). Here: reading and validating token
files, the batch and tick planners, the WAV / FLAC file writers and the device / host pack backends; the run that drives them is decode_files.py.

The mirror image of feeder.py. The split is the same one:

  host    what needs no samples: reading and validating the token files (``num_workers`` files ahead, in order), the segment plan, padding the ragged
          token rows (token bytes are ~1 / 80 of the audio bytes), the RIFF header, the file writes;
  device  everything that touches samples: the decode itself, and the DEVICE WRITER (csrc/pcm_writer.hip: ``at_pcm_peaks`` / ``at_pcm_pack``) that clamps or
          rescales, rounds, narrows to int16 and compacts the valid samples of the padded batch into one buffer — so ONE device-to-host copy per batch
          carries exactly the valid samples at 2 bytes each, into pinned memory on a side stream while the device decodes the next batch and the host
          writes the one before.

Segments mirror how ``encode_batch_files`` cut the audio: every ``chunk_size``-second chunk was encoded as a clip of its own (conv padding and the LSTM
start from zero at every chunk), so every ``chunk_size * 75`` frames are decoded as a clip of their own.
"""
from __future__ import annotations

import ctypes as C
import os
import struct
from dataclasses import dataclass, field
from typing import Iterable, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .audio_io import PCM_LIMIT, pcm16_from_float

HOP = 320                     # samples per frame (24 kHz / 75 Hz)
MIN_FRAMES = 7                # a one-shot decode needs 7 frames: shorter rows are padded up to it and trimmed
PAD_CODE = -1                 # "no code" (include/audiotoken_hip.h, at_encodec_decode): a padded frame is a zero embedding row, as the reference zero-extends short inputs
CODEBOOK_SIZE = 1024
WAV_MAX_DATA = 0xFFFFFFFF - 36    # the RIFF size field is 32 bits: 36 header bytes + data
FLAC_MAX_SAMPLES = (1 << 36) - 1  # STREAMINFO's sample count and the frame header's coded number have 36 bits
FLAC_BLOCK = 4096                 # samples per block (include/audiotoken_hip.h: AT_FLAC_BLOCK); every row ends on one shorter block
AUDIO_FORMATS = ("wav", "flac")
DEFAULT_MAX_HELD_BYTES = 4 << 30  # rescale=True: float rows of a file that stay on the device until its last row is decoded


# ---- token files ------------------------------------------------------------------------------------------------------------------------------------------
class TokenFileError(Exception):
    """A token file ``decode_batch_files`` cannot decode; the message is the reason recorded in ``AudioToken.skipped_files``."""


def read_token_file(path, num_codebooks: int, audio_format: str = "wav") -> np.ndarray:
    """``[K, T]`` int64 codes of a token file (int16 or int64 ``[K, T]`` or ``[1, K, T]``), validated on the host before anything is uploaded."""
    try:
        arr = np.load(str(path), allow_pickle=False)
    except Exception as e:   # noqa: BLE001 — np.load raises ValueError / OSError / EOFError / UnpicklingError depending on how the file is damaged
        raise TokenFileError(f"unreadable token file ({type(e).__name__}: {e})") from e
    if not isinstance(arr, np.ndarray):
        raise TokenFileError("unreadable token file (not a single .npy array)")
    if arr.dtype not in (np.dtype(np.int16), np.dtype(np.int64)):
        raise TokenFileError(f"token dtype {arr.dtype} (int16 or int64 expected)")
    if arr.ndim == 3 and arr.shape[0] == 1:
        arr = arr[0]
    if arr.ndim != 2:
        raise TokenFileError(f"token array of rank {arr.ndim} with shape {tuple(arr.shape)} ([K, T] or [1, K, T] expected)")
    K, T = arr.shape
    if K < 1 or K > int(num_codebooks):
        raise TokenFileError(f"{K} code books, the model has {int(num_codebooks)}")
    if T == 0:
        raise TokenFileError("empty token file (T = 0)")
    lo, hi = int(arr.min()), int(arr.max())
    if lo < 0 or hi >= CODEBOOK_SIZE:
        raise TokenFileError(f"code {lo if lo < 0 else hi} outside [0, {CODEBOOK_SIZE - 1}]")
    if audio_format == "wav" and HOP * 2 * T > WAV_MAX_DATA:
        raise TokenFileError(f"{T} frames would pass the 4 GiB limit of a RIFF file")
    if audio_format == "flac" and HOP * T > FLAC_MAX_SAMPLES:
        raise TokenFileError(f"{T} frames would pass FLAC's limit of 2^36 - 1 samples")
    return np.ascontiguousarray(arr, dtype=np.int64)


def output_path(token_file: str, outdir: str, token_dir: Optional[str], audio_format: str = "wav") -> str:
    """``<stem>.wav`` (``<stem>.flac``): flat in ``outdir`` for a file list, at the mirrored relative path for a directory."""
    stem = os.path.splitext(os.path.basename(token_file))[0]
    rel = ""
    if token_dir is not None:
        rel = os.path.dirname(os.path.relpath(token_file, start=str(token_dir)))
        if rel.startswith("..") or os.path.isabs(rel):
            rel = ""
    return os.path.join(outdir, rel, stem + "." + audio_format)


# ---- the segment plan: a pure function of (K, T) per file ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SegmentRow:
    file: int        # the caller's file id
    t0: int          # first frame of the segment inside the file
    valid: int       # frames of the segment
    last: bool       # the file's last segment


@dataclass
class BatchPlan:
    """One decode call: ``rows`` of equal K, right-padded to ``t_max`` frames. Row b of the decoder's output starts at float ``src_off[b]`` and has
    ``n[b]`` real samples; packed, the rows follow each other without gaps from ``dst_off[b]``."""
    K: int
    rows: List[SegmentRow]
    t_max: int = 0
    src_off: List[int] = field(default_factory=list)
    dst_off: List[int] = field(default_factory=list)
    n: List[int] = field(default_factory=list)
    total: int = 0

    def finish(self) -> "BatchPlan":
        self.t_max = max(MIN_FRAMES, max(r.valid for r in self.rows))
        self.src_off = [b * HOP * self.t_max for b in range(len(self.rows))]
        self.n = [HOP * r.valid for r in self.rows]
        self.dst_off = [0] * len(self.rows)
        pos = 0
        for b, n in enumerate(self.n):
            self.dst_off[b] = pos
            pos += n
        self.total = pos
        return self


def chunk_frames_of(chunk_size, token_rate: int = 75) -> Optional[int]:
    return None if chunk_size is None else max(1, int(round(chunk_size * token_rate)))


def plan_batches(files: Iterable[Tuple[int, int, int]], batch_size: int, chunk_frames: Optional[int]) -> Iterator[BatchPlan]:
    """``files`` = (id, K, T) in order -> the decode calls. A file is cut into segments of ``chunk_frames`` frames (None: one segment); consecutive segments of
    equal K fill batches of up to ``batch_size`` rows; a change of K closes the batch. Lazy: a batch is yielded as soon as it is full."""
    assert batch_size >= 1 and (chunk_frames is None or chunk_frames >= 1)
    rows: List[SegmentRow] = []
    K_open = None
    for fid, K, T in files:
        assert K >= 1 and T >= 1
        if rows and K != K_open:
            yield BatchPlan(K_open, rows).finish()
            rows = []
        K_open = K
        step = T if chunk_frames is None else chunk_frames
        for t0 in range(0, T, step):
            valid = min(step, T - t0)
            rows.append(SegmentRow(fid, t0, valid, t0 + valid == T))
            if len(rows) == batch_size:
                yield BatchPlan(K_open, rows).finish()
                rows = []
    if rows:
        yield BatchPlan(K_open, rows).finish()


def plan_ticks(lengths: Iterable[int], batch_size: int, step: Optional[int]) -> Iterator[List[SegmentRow]]:
    """The tick plan of a streamed run, shared by both directions: ``lengths`` = units per file in order (frames of a token file, chunks of
    an audio file), at most ``batch_size`` files live at once, every live file contributes its next ``step`` units per tick (None: all of them). A file
    whose units are exhausted leaves with that tick, and its place goes to the next file at the start of the next one. A tick is the list of its rows in
    file order; ``SegmentRow.file`` counts the files from 0. Lazy: the next length is read only when a place is free."""
    assert batch_size >= 1 and (step is None or step >= 1)
    it = enumerate(lengths)
    live: List[list] = []     # [file, units, position]
    while True:
        while len(live) < batch_size:
            nxt = next(it, None)
            if nxt is None:
                break
            assert nxt[1] >= 1, "a file without units has no tick"
            live.append([nxt[0], int(nxt[1]), 0])
        if not live:
            return
        tick = []
        for f in live:
            valid = f[1] - f[2] if step is None else min(step, f[1] - f[2])
            tick.append(SegmentRow(f[0], f[2], valid, f[2] + valid == f[1]))
            f[2] += valid
        live = [f for f in live if f[2] < f[1]]
        yield tick


def plan_stream_ticks(files: Iterable[Tuple[int, int]], batch_size: int, chunk_frames: Optional[int]) -> Iterator[List[SegmentRow]]:
    """``decode_batch_files(stream=True)``: ``files`` = (K, T) in order -> ticks of (file, first frame, frames, last). K plays no part in who is live: the
    pool forms one group per (phase, K, frames) inside a tick."""
    return plan_ticks((T for _, T in files), batch_size, chunk_frames)


def plan_encode_stream_ticks(files: Iterable[Sequence[int]], batch_size: int) -> Iterator[List[SegmentRow]]:
    """``encode_batch_files(stream=True)``: ``files`` = the sample counts of every file's chunks, known once the file is opened -> ticks of (file, chunk
    index, 1, last): one chunk per live file and tick."""
    return plan_ticks((len(chunks) for chunks in files), batch_size, 1)


def padded_tokens(plan: BatchPlan, tokens_of) -> torch.Tensor:
    """The ``[B, K, t_max]`` int64 batch of a plan, rows right-padded with ``PAD_CODE``; ``tokens_of(file id)`` = that file's ``[K, T]`` array."""
    out = np.full((len(plan.rows), plan.K, plan.t_max), PAD_CODE, dtype=np.int64)
    for b, r in enumerate(plan.rows):
        out[b, :, :r.valid] = tokens_of(r.file)[:, r.t0:r.t0 + r.valid]
    return torch.from_numpy(out)


# ---- the WAV file ---------------------------------------------------------------------------------------------------------------------------------------------
class WavTooLarge(Exception):
    pass


class WavWriter:
    """Plain RIFF PCM, mono, 16 bit. The samples go to ``<path>.part``; ``close`` patches the two header sizes and moves the file into place (replacing an
    existing one), ``abort`` removes it: ``path`` either holds a complete file or is untouched."""

    def __init__(self, path, sample_rate: int):
        self.path = str(path)
        self.tmp = self.path + ".part"
        self.sample_rate = int(sample_rate)
        self.data_bytes = 0
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        self._f = open(self.tmp, "wb")
        self._f.write(self._header(0))

    def _header(self, data_bytes: int) -> bytes:
        sr = self.sample_rate
        return (b"RIFF" + struct.pack("<I", 36 + data_bytes) + b"WAVE" + b"fmt " + struct.pack("<IHHIIHH", 16, 1, 1, sr, sr * 2, 2, 16)
                + b"data" + struct.pack("<I", data_bytes))

    def write(self, pcm) -> None:
        """``pcm``: int16 samples (an array, or a bytes-like of little-endian int16)."""
        buf = memoryview(np.ascontiguousarray(pcm, dtype="<i2")).cast("B") if isinstance(pcm, np.ndarray) else memoryview(pcm).cast("B")
        if self.data_bytes + len(buf) > WAV_MAX_DATA:
            raise WavTooLarge(f"{self.path}: more than 4 GiB")
        self._f.write(buf)
        self.data_bytes += len(buf)

    def close(self) -> None:
        f, self._f = self._f, None
        try:
            f.seek(4)
            f.write(struct.pack("<I", 36 + self.data_bytes))
            f.seek(40)
            f.write(struct.pack("<I", self.data_bytes))
            f.close()
            os.replace(self.tmp, self.path)
        except BaseException:
            self._f = f
            self.abort()
            raise

    def abort(self) -> None:
        f, self._f = self._f, None
        try:
            if f is not None and not f.closed:
                f.close()
        finally:
            try:
                os.remove(self.tmp)
            except OSError:
                pass


# ---- the FLAC file ------------------------------------------------------------------------------------------------------------------------------------------------
class FlacTooLarge(Exception):
    pass


def flac_encode_pcm16(rows: Sequence[np.ndarray]) -> Tuple[np.ndarray, np.ndarray]:
    """The HOST twin of the device encoder (``at_flac_encode_pcm16``): int16 rows -> ``(block records, compacted subframe bytes)`` in the layout
    ``at_flac_encode_rows`` produces (records in row order, ``byte_off`` the exclusive prefix sum of ``nbytes``). ctypes releases the GIL."""
    from . import _cabi
    lib = _cabi.load()
    rows = [np.ascontiguousarray(r, dtype=np.int16).reshape(-1) for r in rows]
    nblocks = sum((len(r) + FLAC_BLOCK - 1) // FLAC_BLOCK for r in rows)
    cap = nblocks + 2 * sum(len(r) for r in rows)
    recs = np.zeros(nblocks, dtype=_cabi.FLAC_BLOCK_DTYPE)
    data = np.zeros(max(cap, 1), dtype=np.uint8)
    b = off = 0
    for j, r in enumerate(rows):
        nb = lib.at_flac_encode_pcm16(r.ctypes.data, len(r), j, recs.ctypes.data + b * recs.itemsize, nblocks - b, data.ctypes.data, cap, off)
        if nb < 0:
            raise _cabi.HipLibraryError(f"at_flac_encode_pcm16 failed: {_cabi.last_error()}")
        b += nb
        if nb:
            off = int(recs["byte_off"][b - 1]) + int(recs["nbytes"][b - 1])
    return recs, data[:off]


def flac_frames(recs: np.ndarray, data: np.ndarray, sample_rate: int, first_sample_of_row) -> Tuple[np.ndarray, np.ndarray]:
    """``at_flac_write_frames``: the records' frames (header + CRC-8, subframe, CRC-16) back to back, and the call's stats for ``FlacWriter.write``."""
    from . import _cabi
    lib = _cabi.load()
    if len(recs) == 0:
        return np.zeros(0, dtype=np.uint8), np.zeros(7, dtype=np.int64)
    recs = np.ascontiguousarray(recs)
    first = np.ascontiguousarray(first_sample_of_row, dtype=np.int64)
    cap = int(recs["nbytes"].sum()) + 18 * len(recs)
    out = np.empty(max(cap, 1), dtype=np.uint8)
    stats = np.zeros(7, dtype=np.int64)
    n = lib.at_flac_write_frames(recs.ctypes.data, len(recs), data.ctypes.data, len(data), int(sample_rate), first.ctypes.data, len(first), out.ctypes.data, cap,
                                 stats.ctypes.data)
    if n < 0:
        raise _cabi.HipLibraryError(f"at_flac_write_frames failed: {_cabi.last_error()}")
    return out[:n], stats


class FlacWriter:
    """FLAC (RFC 9639), mono, 16 bit, variable block size; the ``WavWriter`` contract. The frames go to ``<path>.part`` behind 42 reserved bytes; ``close``
    writes the stream head there (STREAMINFO: block and frame size ranges, the sample count; MD5 zero = not computed) and moves the file into place,
    ``abort`` removes it: ``path`` either holds a complete file or is untouched. ``samples`` is the index the next row's first sample gets."""

    def __init__(self, path, sample_rate: int):
        self.path = str(path)
        self.tmp = self.path + ".part"
        self.sample_rate = int(sample_rate)
        self.samples = 0
        self.data_bytes = 42
        self._min_frame = self._max_frame = self._min_block = self._max_block = self._last_block = 0
        os.makedirs(os.path.dirname(os.path.abspath(self.path)), exist_ok=True)
        self._f = open(self.tmp, "wb")
        self._f.write(bytes(42))

    def write(self, frames, stats) -> None:
        """``frames`` / ``stats``: what ``at_flac_write_frames`` returned for the next blocks of the stream (coded from sample ``self.samples`` on)."""
        min_frame, max_frame, min_block, max_block, last_block, nframes, nsamples = (int(x) for x in stats)
        if nframes == 0:
            return
        if self.samples + nsamples > FLAC_MAX_SAMPLES:
            raise FlacTooLarge(f"{self.path}: more than 2^36 - 1 samples")
        self._f.write(memoryview(frames).cast("B"))
        self.data_bytes += len(frames)
        # STREAMINFO's minimum is over the blocks but the stream's last: the last block so far stops being the last
        for b in (self._last_block, min_block):
            if b:
                self._min_block = b if not self._min_block else min(self._min_block, b)
        self._max_block = max(self._max_block, max_block)
        self._last_block = last_block
        self._min_frame = min_frame if not self._min_frame else min(self._min_frame, min_frame)
        self._max_frame = max(self._max_frame, max_frame)
        self.samples += nsamples

    def close(self) -> None:
        from . import _cabi
        f, self._f = self._f, None
        try:
            head = (C.c_uint8 * 42)()
            _cabi.check(_cabi.load().at_flac_streaminfo(self.sample_rate, self._min_block or self._last_block, self._max_block, self._min_frame,
                                                       self._max_frame, self.samples, head), "at_flac_streaminfo")
            f.seek(0)
            f.write(bytes(head))
            f.close()
            os.replace(self.tmp, self.path)
        except BaseException:
            self._f = f
            self.abort()
            raise

    def abort(self) -> None:
        WavWriter.abort(self)


def open_writer(path, sample_rate: int, audio_format: str):
    return FlacWriter(path, sample_rate) if audio_format == "flac" else WavWriter(path, sample_rate)


# ---- float rows -> int16, on the device or (device_writer=False) on the host -------------------------------------------------------------------------------------
PackRow = Tuple[int, int, int, float]     # (src_off, dst_off, n, scale)


class _Packed:
    """The int16 samples and per-row ``[clipped, non-finite]`` counts of one pack, possibly still on their way to the host."""

    def __init__(self, pcm=None, counts=None, buf=None, event=None, pool=None, total=0, nrows=0, counts_at=0):
        self._pcm, self._counts, self._buf, self._event, self._pool = pcm, counts, buf, event, pool
        self._total, self._nrows, self._counts_at = total, nrows, counts_at

    def result(self):
        if self._event is not None:
            self._event.synchronize()
            self._event = None
            host = self._buf.numpy()
            self._pcm = host[:2 * self._total].view(np.int16)
            self._counts = host[self._counts_at:self._counts_at + 8 * self._nrows].view(np.uint32).reshape(self._nrows, 2)
        return self._pcm, self._counts

    def write_row(self, writer, j: int, d: int, n: int) -> None:
        """Row ``j`` of the pack (``n`` samples from packed sample ``d``) into its file's writer."""
        writer.write(self.result()[0][d:d + n])

    def release(self) -> None:
        if self._buf is not None:
            if self._event is not None:
                self._event.synchronize()
                self._event = None
            self._pool.give(self._buf)
            self._buf = self._pcm = self._counts = None


class _FlacPacked:
    """The block records, compacted subframe bytes and per-row counts of one FLAC pack. From the device the records and counts come first; ``result`` —
    where the host may wait, one batch later — reads the total from them and brings EXACTLY the compacted bytes."""

    def __init__(self, recs=None, data=None, counts=None, sample_rate=0, owner=None, head=None, head_event=None, dev=None, bytes_at=0, nblocks=0, nrows=0):
        self._recs, self._data, self._counts, self.sample_rate = recs, data, counts, sample_rate
        self._owner, self._head, self._event, self._dev, self._bytes_at, self._nblocks, self._nrows = owner, head, head_event, dev, bytes_at, nblocks, nrows
        self._body = None
        self._row_at = None

    def result(self):
        if self._event is not None:
            o = self._owner
            self._event.synchronize()
            self._event = None
            host = self._head.numpy()
            from . import _cabi
            self._recs = host[:40 * self._nblocks].view(_cabi.FLAC_BLOCK_DTYPE)
            self._counts = host[40 * self._nblocks:40 * self._nblocks + 8 * self._nrows].view(np.uint32).reshape(self._nrows, 2)
            total = int(self._recs["byte_off"][-1]) + int(self._recs["nbytes"][-1])
            assert 0 < total <= self._dev.numel() - self._bytes_at, "the device encoder's byte count is outside its buffer"
            self._body = o._pool.take(total)
            with torch.cuda.device(o.device), torch.cuda.stream(o.copy_stream):
                self._body[:total].copy_(self._dev[self._bytes_at:self._bytes_at + total], non_blocking=True)
            o.copy_stream.synchronize()
            self._dev = None
            o.bytes_downloaded += total
            self._data = self._body.numpy()[:total]
        if self._row_at is None:
            self._row_at = np.searchsorted(self._recs["row"], np.arange(self._counts.shape[0] + 1))      # records are in row order
        return self._recs, self._data, self._counts

    def write_row(self, writer, j: int, d: int, n: int) -> None:
        recs, data, _ = self.result()
        mine = recs[self._row_at[j]:self._row_at[j + 1]]
        assert int(mine["n"].sum()) == n, "the encoder's blocks do not add up to the row"
        first = np.zeros(self._counts.shape[0], dtype=np.int64)
        first[j] = writer.samples
        writer.write(*flac_frames(mine, data, self.sample_rate, first))

    def release(self) -> None:
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        for buf in (self._head, self._body):
            if buf is not None:
                self._owner._pool.give(buf)
        self._head = self._body = self._dev = self._recs = self._data = self._counts = None


class DeviceWriter:
    """``at_pcm_peaks`` / ``at_pcm_pack`` on the decoder's stream, then the packed buffer's copy into pinned memory on a side stream."""

    def __init__(self, device):
        from . import _cabi
        from .feeder import _POOL
        self._cabi = _cabi
        self.lib = _cabi.load()
        self.device = torch.device(device)
        assert self.device.type == "cuda", "the device writer needs a HIP device"
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self._pool = _POOL
        self.bytes_downloaded = 0

    def hold(self, wav: torch.Tensor):
        return wav.reshape(-1)

    def _descs(self, rows: Sequence[PackRow], src_numel: int) -> torch.Tensor:
        for s, d, n, _ in rows:
            assert 0 <= s and s + n <= src_numel and d >= 0 and n >= 0, "pack row outside the decoder's output"
        arr = (self._cabi.PcmRowDesc * len(rows))(*[self._cabi.PcmRowDesc(int(s), int(d), int(n), float(sc), 0) for s, d, n, sc in rows])
        return torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(self.device)

    def peaks(self, held: torch.Tensor, rows: Sequence[PackRow]) -> np.ndarray:
        if not rows:
            return np.zeros(0, np.float32)
        with torch.cuda.device(self.device):
            descs = self._descs(rows, held.numel())
            out = torch.empty(len(rows), dtype=torch.float32, device=self.device)
            self._cabi.check(self.lib.at_pcm_peaks(held.data_ptr(), descs.data_ptr(), len(rows), max(r[2] for r in rows), out.data_ptr(),
                                                   self._cabi.current_stream_handle(self.device)), "at_pcm_peaks")
            return out.cpu().numpy()

    def pack(self, held: torch.Tensor, rows: Sequence[PackRow]) -> _Packed:
        total = sum(r[2] for r in rows)
        if not rows or total == 0:
            return _Packed(np.zeros(0, np.int16), np.zeros((len(rows), 2), np.uint32))
        assert all(d + n <= total for _, d, n, _ in rows), "pack row outside the packed buffer"
        counts_at = (2 * total + 15) // 16 * 16
        nbytes = counts_at + 8 * len(rows)
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            descs = self._descs(rows, held.numel())
            dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._cabi.check(self.lib.at_pcm_pack(held.data_ptr(), descs.data_ptr(), len(rows), max(r[2] for r in rows), float(PCM_LIMIT), dev.data_ptr(),
                                                  dev.data_ptr() + counts_at, C.c_void_p(main.cuda_stream)), "at_pcm_pack")
            packed = torch.cuda.Event()
            packed.record(main)
            buf = self._pool.take(nbytes)
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(packed)
                buf[:nbytes].copy_(dev, non_blocking=True)
                done = torch.cuda.Event()
                done.record(self.copy_stream)
            dev.record_stream(self.copy_stream)
        self.bytes_downloaded += nbytes
        return _Packed(buf=buf, event=done, pool=self._pool, total=total, nrows=len(rows), counts_at=counts_at)


def _flac_rows(rows: Sequence["PackRow"]):
    """(descriptor tuples (src_off, n, first_block, scale), blocks) of a pack's rows."""
    out, nblocks = [], 0
    for s, _, n, sc in rows:
        out.append((int(s), int(n), nblocks, float(sc)))
        nblocks += (int(n) + FLAC_BLOCK - 1) // FLAC_BLOCK
    return out, nblocks


class DeviceFlacWriter(DeviceWriter):
    """``audio_format="flac"``: ``hold`` / ``peaks`` as the PCM writer; ``pack`` launches ``at_flac_encode_rows`` on the decoder's stream and sends the block
    records and counts to pinned memory on the side stream; the compacted bytes follow in ``_FlacPacked.result``."""

    def __init__(self, device, sample_rate: int):
        super().__init__(device)
        self.sample_rate = int(sample_rate)

    def pack(self, held: torch.Tensor, rows: Sequence[PackRow]) -> _FlacPacked:
        total = sum(r[2] for r in rows)
        if not rows or total == 0:
            return _FlacPacked(np.zeros(0, self._cabi.FLAC_BLOCK_DTYPE), np.zeros(0, np.uint8), np.zeros((len(rows), 2), np.uint32), self.sample_rate)
        descs, nblocks = _flac_rows(rows)
        for s, n, _, _ in descs:
            assert 0 <= s and n >= 0 and s + n <= held.numel(), "pack row outside the decoder's output"
        head_bytes = 40 * nblocks + 8 * len(rows)
        bytes_at = (head_bytes + 15) // 16 * 16
        cap = nblocks + 2 * total                                          # the worst case: every block VERBATIM
        main = torch.cuda.current_stream(self.device)
        with torch.cuda.device(self.device):
            arr = (self._cabi.FlacRowDesc * len(descs))(*[self._cabi.FlacRowDesc(*d) for d in descs])
            descs_dev = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(self.device)
            dev = torch.empty(bytes_at + cap, dtype=torch.uint8, device=self.device)
            ws_bytes = int(self.lib.at_flac_encode_workspace_bytes(nblocks))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
            self._cabi.check(self.lib.at_flac_encode_rows(held.data_ptr(), descs_dev.data_ptr(), len(rows), nblocks, float(PCM_LIMIT), dev.data_ptr(),
                                                          dev.data_ptr() + bytes_at, cap, dev.data_ptr() + 40 * nblocks, ws.data_ptr(), ws_bytes,
                                                          C.c_void_p(main.cuda_stream)), "at_flac_encode_rows")
            packed = torch.cuda.Event()
            packed.record(main)
            head = self._pool.take(head_bytes)
            with torch.cuda.stream(self.copy_stream):
                self.copy_stream.wait_event(packed)
                head[:head_bytes].copy_(dev[:head_bytes], non_blocking=True)
                done = torch.cuda.Event()
                done.record(self.copy_stream)
            dev.record_stream(self.copy_stream)
        self.bytes_downloaded += head_bytes
        return _FlacPacked(sample_rate=self.sample_rate, owner=self, head=head, head_event=done, dev=dev, bytes_at=bytes_at, nblocks=nblocks, nrows=len(rows))


class HostWriter:
    """``device_writer=False``: the float batch comes to the host and numpy applies the same rule (audio_io.pcm16_from_float) — the comparison path."""

    def __init__(self, device=None):
        self.bytes_downloaded = 0

    def hold(self, wav: torch.Tensor):
        x = wav.detach().reshape(-1).cpu().numpy()
        self.bytes_downloaded += x.nbytes
        return x

    def peaks(self, held: np.ndarray, rows: Sequence[PackRow]) -> np.ndarray:
        from .audio_io import finite_peak
        return np.array([finite_peak(held[s:s + n]) for s, _, n, _ in rows], dtype=np.float32)

    def pack(self, held: np.ndarray, rows: Sequence[PackRow]) -> _Packed:
        pcm = np.zeros(sum(r[2] for r in rows), dtype=np.int16)
        counts = np.zeros((len(rows), 2), dtype=np.uint32)
        for i, (s, d, n, scale) in enumerate(rows):
            pcm[d:d + n], counts[i, 0], counts[i, 1] = pcm16_from_float(held[s:s + n], np.float32(scale))
        return _Packed(pcm, counts)


class HostFlacWriter(HostWriter):
    """``device_writer=False`` with ``audio_format="flac"``: numpy quantises, the host twin of the encoder (``at_flac_encode_pcm16``) compresses."""

    def __init__(self, device=None, sample_rate: int = 0):
        super().__init__(device)
        self.sample_rate = int(sample_rate)

    def pack(self, held: np.ndarray, rows: Sequence[PackRow]) -> _FlacPacked:
        counts = np.zeros((len(rows), 2), dtype=np.uint32)
        pcm = []
        for i, (s, _, n, scale) in enumerate(rows):
            q, counts[i, 0], counts[i, 1] = pcm16_from_float(held[s:s + n], np.float32(scale))
            pcm.append(q)
        recs, data = flac_encode_pcm16(pcm)
        return _FlacPacked(recs, data, counts, self.sample_rate)


# ---- the run: decode_files.py ------------------------------------------------------------------------------------------------------------------------------------
def decode_files(tok, inputs, *args, **kwargs) -> None:
    """``decode_files.decode_files``, under the name it had when it lived here (that module imports this one)."""
    from .decode_files import decode_files as run
    run(tok, inputs, *args, **kwargs)
