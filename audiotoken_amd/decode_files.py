"""The run behind ``AudioToken.decode_batch_files``: ``DecodeRun`` takes (token file, output path) pairs through the planners, the
decoder and the pack backends of writer.py into WAV / FLAC files.

Its state is small and explicit: ``files`` (what is known of every valid input), ``held`` (batches decoded but not packed: ``rescale=True`` waits for the
last row of a file), ``pending`` (packs on their way to the host, not yet written), ``summary`` and the ``backend``. The guarantees it keeps: a half-written
audio file is removed, a dropped file never gets a row, and what was verified and packed before a failing decode is still written."""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from .audio_io import rescale_factor
from .prefetch import ordered_map
from .runs import RunLog
from .writer import (AUDIO_FORMATS, HOP, MIN_FRAMES, PAD_CODE, BatchPlan, DeviceFlacWriter, DeviceWriter, FlacTooLarge, HostFlacWriter, HostWriter,
                     SegmentRow, TokenFileError, WavTooLarge, chunk_frames_of, open_writer, padded_tokens, plan_batches, plan_stream_ticks, read_token_file)


@dataclass
class _File:
    path: str
    out: str
    tokens: Optional[np.ndarray] = None
    rows_left: int = 0                  # segments not yet decoded
    peak: np.float32 = np.float32(0.0)  # rescale=True: max over the rows decoded so far
    held_bytes: int = 0
    dropped: bool = False               # skipped after its first row was planned (max_held_bytes, a write error)
    writer: Optional[object] = None     # WavWriter / FlacWriter
    written: bool = False


class DecodeRun:
    """One ``decode_batch_files`` call: ``inputs`` = (token file, output path) in order. ``tok`` supplies ``decoder`` (``forward`` / ``verified``),
    ``device``, ``skipped_files``; ``run_summary`` / ``run_timings`` are left on it.

    Chunked (``run_batches``), per batch k in this order: ``forward`` (asynchronous on the device); ``write_pending`` — the batches before, whose copies
    ran behind the decode before this one; read / pad / upload batch k + 1; ``verified``; ``hold``; ``release_held``.

    ``stream=True`` (``run_ticks``): every file is ONE clip. Up to ``batch_size`` files are live, one slot of a decode stream pool each
    (``decoder.new_stream_pool``); per tick (``plan_stream_ticks``) every live file pushes its next ``chunk_size * 75`` frames and the pool batches the rows
    of equal phase, K and length. The audio of a tick goes through the same writers as a batch's; a file below 7 frames is padded with ``PAD_CODE`` and
    trimmed, as the segments of the chunked route are."""
    BATCH_LAPS = ("encode_call_s", "save_s", "stage_s", "device_wait_s")
    TICK_LAPS = ("stage_s", "encode_call_s", "save_s", "device_wait_s")

    def __init__(self, tok, inputs: Sequence[Tuple[str, str]], batch_size: int, chunk_size, num_workers: int, rescale: bool, device_writer: bool,
                 max_held_bytes: int, sample_rate: int, token_rate: int, audio_format: str = "wav", stream: bool = False, log: Optional[RunLog] = None,
                 decoder=None):
        """``decoder``: the acoustic decoder to run when it is not ``tok``'s own (semantic_files.py: the semantic tokenizers have none)."""
        self.log = log or RunLog(tok, "decode_batch_files", "audio")     # (the caller's, when it already had inputs to skip)
        self.tok, self.inputs, self.batch_size, self.num_workers, self.rescale, self.stream = tok, inputs, batch_size, num_workers, rescale, stream
        self.max_held_bytes, self.sample_rate, self.audio_format = max_held_bytes, sample_rate, audio_format
        self.chunk_frames = chunk_frames_of(chunk_size, token_rate)
        self.dec = dec = decoder if decoder is not None else tok.decoder
        self.device = device = torch.device(tok.device)
        self.num_codebooks = int(getattr(getattr(dec, "_h", None), "n_codebooks", tok.num_codebooks))
        assert audio_format in AUDIO_FORMATS
        if audio_format == "flac":
            self.backend = DeviceFlacWriter(device, sample_rate) if device_writer else HostFlacWriter(device, sample_rate)
        else:
            self.backend = DeviceWriter(device) if device_writer else HostWriter(device)
        self.fb0 = getattr(dec, "fallback_batches", 0)
        self.summary = tok.run_summary = {"files": 0, "segments": 0, "batches": 0, "fallback_batches": 0, "clipped_samples": 0, "nonfinite_samples": 0,
                                          "skipped_files": 0, "audio_bytes": 0}
        tok.run_timings = self.log.timings
        self.files: dict = {}           # input index -> _File, of the valid inputs read so far
        self.held: List[list] = []      # [plan, float rows (device tensor / host array)] decoded but not packed
        self.pending: List[tuple] = []  # (plan rows packed, _Packed): packed, on their way to the host, not yet written

    # ---- the inputs ---------------------------------------------------------------------------------------------------------------------------------------
    def load(self, item):
        i, (path, out) = item
        try:
            return i, path, out, read_token_file(path, self.num_codebooks, self.audio_format), None
        except TokenFileError as e:
            return i, path, out, None, str(e)

    def valid_files(self):
        """(input index, K, T) of every readable token file, ``num_workers`` files read ahead, in order; the others are skipped."""
        for i, path, out, tokens, why in ordered_map(self.load, list(enumerate(self.inputs)), self.num_workers):
            if tokens is None:
                self.log.skipped(path, why)
                continue
            K, T = tokens.shape
            step = self.chunk_frames
            self.files[i] = _File(path, out, tokens, rows_left=1 if step is None else (T + step - 1) // step)
            yield i, K, T

    def drop(self, f: _File, why: str) -> None:
        if not f.dropped:
            f.dropped = True
            if f.writer is not None:
                f.writer.abort()
                f.writer = None
            self.log.skipped(f.path, why)

    # ---- decoded rows -> files ----------------------------------------------------------------------------------------------------------------------------
    def write_row(self, f: _File, packed, j: int, r: SegmentRow, d: int, n: int, counts) -> None:
        summary = self.summary
        try:
            if f.writer is None:
                f.writer = open_writer(f.out, self.sample_rate, self.audio_format)
            packed.write_row(f.writer, j, d, n)
            summary["clipped_samples"] += int(counts[j, 0])
            summary["nonfinite_samples"] += int(counts[j, 1])
            if r.last:
                w, f.writer = f.writer, None
                w.close()
                f.written = True
                summary["files"] += 1
                summary["audio_bytes"] += (44 if self.audio_format == "wav" else 0) + w.data_bytes
        except (OSError, WavTooLarge, FlacTooLarge) as e:
            self.drop(f, f"cannot write {f.out}: {type(e).__name__}: {e}")

    def write_pending(self) -> None:
        pending = self.pending
        while pending:
            rows, packed = pending.pop(0)
            try:
                counts = packed.result()[-1]
                for j, (r, d, n) in enumerate(rows):
                    f = self.files[r.file]
                    if not f.dropped:
                        self.write_row(f, packed, j, r, d, n, counts)
            finally:
                packed.release()

    def hold(self, plan: BatchPlan, wav, row_bytes, decoded: bool) -> None:
        """The float rows of a decode call join ``held``; with ``rescale`` their peaks go into their files, and a file that holds more than
        ``max_held_bytes`` is dropped. ``row_bytes(b)``: what row b keeps on the device. ``decoded``: these rows count as decoded here (the chunked run; the
        streamed run counted them when it planned the tick)."""
        files, rescale, backend = self.files, self.rescale, self.backend
        rows_f = backend.hold(wav)
        if rescale:
            pk = backend.peaks(rows_f, [(plan.src_off[b], 0, plan.n[b], 1.0) for b in range(len(plan.rows))])
        for b, r in enumerate(plan.rows):
            f = files[r.file]
            if decoded:
                f.rows_left -= 1
            if rescale and not f.dropped:
                f.peak = max(f.peak, np.float32(pk[b]))
                f.held_bytes += row_bytes(b)
                if f.held_bytes > self.max_held_bytes:
                    self.drop(f, "rescale=True holds the file's float rows on the device until its last row: more than max_held_bytes = "
                                 f"{self.max_held_bytes}")
        self.held.append([plan, rows_f])

    def release_held(self) -> None:
        """Pack every held batch whose files are all complete (clamp mode: every batch, at once), in order."""
        files, held, rescale = self.files, self.held, self.rescale
        while held:
            plan, rows_f = held[0]
            # (batches are in file order, so only the LAST row's file can be incomplete; a tick of a streamed run has a row of every live file)
            if rescale and any(files[r.file].rows_left > 0 and not files[r.file].dropped for r in (plan.rows if self.stream else plan.rows[-1:])):
                break
            held.pop(0)
            keep, pack_rows, pos = [], [], 0
            for b, r in enumerate(plan.rows):
                f = files[r.file]
                if f.dropped:
                    continue
                keep.append((r, pos, plan.n[b]))
                pack_rows.append((plan.src_off[b], pos, plan.n[b], float(rescale_factor(f.peak)) if rescale else 1.0))
                pos += plan.n[b]
            if keep:
                self.pending.append((keep, self.backend.pack(rows_f, pack_rows)))
            for r in plan.rows:
                if r.last:      # (no later batch holds a row of it)
                    files[r.file].tokens = None

    # ---- the chunked run ----------------------------------------------------------------------------------------------------------------------------------
    def next_batch(self, plans):
        """(plan, its tokens on the device) of the next batch, or (None, None): reads the token files the plan reaches, pads, uploads."""
        plan = next(plans, None)
        return plan, (padded_tokens(plan, lambda i: self.files[i].tokens).to(self.device) if plan is not None else None)

    def run_batches(self) -> None:
        dec, log = self.dec, self.log
        plans = plan_batches(self.valid_files(), self.batch_size, self.chunk_frames)
        t0 = time.perf_counter()
        plan, toks = self.next_batch(plans)
        log.lap("stage_s", t0)
        while plan is not None:
            t0 = time.perf_counter()
            wav = dec.forward(toks)                           # asynchronous on the device
            t1 = time.perf_counter()
            self.write_pending()                              # the batches before: their copies ran behind the decode before this one
            t2 = time.perf_counter()
            nxt, nxt_toks = self.next_batch(plans)            # the next batch's tokens are read / padded / uploaded while this one decodes
            t3 = time.perf_counter()
            if hasattr(dec, "verified"):
                wav = dec.verified(wav, toks)                 # the correctness ladder: no audio is accepted before the call's status was read
            self.hold(plan, wav, lambda b: 4 * HOP * plan.t_max, decoded=True)
            del wav
            self.release_held()
            log.laps(self.BATCH_LAPS, t0, t1, t2, t3, time.perf_counter())
            self.count(len(plan.rows))
            plan, toks = nxt, nxt_toks

    def count(self, rows: int) -> None:
        self.log.batch(rows)
        self.summary["batches"] += 1
        self.summary["segments"] += rows

    # ---- the streamed run -----------------------------------------------------------------------------------------------------------------------------------
    def tick_feed(self, tick, order, sids, pool):
        """(rows of the tick by input index, {stream id: frames}, {input index: samples to keep}): the live files' next frames; a file on its first tick
        gets its slot, a dropped one gives it back."""
        rows, feed, trim = [], {}, {}
        for r in tick:
            i = order[r.file]
            f = self.files[i]
            f.rows_left -= 1
            if f.dropped:
                if i in sids:
                    pool.close(sids.pop(i))
                continue
            if i not in sids:
                sids[i] = pool.open()
            x = f.tokens[:, r.t0:r.t0 + r.valid]
            if r.last and r.t0 + r.valid < MIN_FRAMES:     # the whole file is below a first push's 7 frames: "no code" frames behind it, cut off again below
                trim[i] = HOP * (r.t0 + r.valid)
                x = np.concatenate([x, np.full((x.shape[0], MIN_FRAMES - (r.t0 + r.valid)), PAD_CODE, dtype=np.int64)], axis=1)
            feed[sids[i]] = torch.from_numpy(np.ascontiguousarray(x))
            rows.append(SegmentRow(i, r.t0, r.valid, r.last))
        return rows, feed, trim

    def hold_tick(self, rows, outs) -> None:
        emitted = [(r, o) for r, o in zip(rows, outs) if o.numel() > 0]    # (a file's first ticks emit nothing while it holds fewer than 7 frames)
        if emitted:
            plan = BatchPlan(0, [r for r, _ in emitted])
            plan.n = [int(o.numel()) for _, o in emitted]
            plan.src_off = plan.dst_off = [sum(plan.n[:b]) for b in range(len(plan.n))]
            plan.total = sum(plan.n)
            self.hold(plan, torch.cat([o for _, o in emitted]), lambda b: 4 * plan.n[b], decoded=False)

    def run_ticks(self) -> None:
        """The streamed run. A tick: upload and push the live files' next frames (the pool reads every group's status word: the audio is verified when
        ``push`` returns), write what the ticks before packed, then hold / pack this tick's audio as a batch's."""
        log = self.log
        pool = self.dec.new_stream_pool(self.batch_size)
        order: List[int] = []      # position in the tick plan -> file id

        def shapes():
            for i, K, T in self.valid_files():
                order.append(i)
                yield K, T

        sids: dict = {}
        for tick in plan_stream_ticks(shapes(), self.batch_size, self.chunk_frames):
            t0 = time.perf_counter()
            rows, feed, trim = self.tick_feed(tick, order, sids, pool)
            t1 = time.perf_counter()
            out = pool.push(feed) if feed else {}
            outs = [out[sids[r.file]][:trim.get(r.file)] for r in rows]
            done = [sids.pop(r.file) for r in rows if r.last]
            if done:
                pool.flush(done)                                # started streams hold nothing: this frees their slots
            t2 = time.perf_counter()
            self.write_pending()
            t3 = time.perf_counter()
            self.hold_tick(rows, outs)
            del out, outs
            self.release_held()
            log.laps(self.TICK_LAPS, t0, t1, t2, t3, time.perf_counter())
            self.count(len(rows))
        self.summary["library_pushes"] = pool.library_pushes

    # ---- the run ------------------------------------------------------------------------------------------------------------------------------------------
    def run(self) -> None:
        ok = False
        try:
            if self.stream:
                self.run_ticks()
            else:
                self.run_batches()
            t0 = time.perf_counter()
            self.write_pending()
            self.log.lap("save_s", t0)
            ok = True
        finally:
            self.finish(ok)
        self.log.report()

    def finish(self, ok: bool) -> None:
        """Also when a decode raised: what was verified and packed before it belongs in its files; then every file still open is incomplete and is removed."""
        if not ok:
            with self.log.guard("writing the batches before the failure failed too"):
                self.write_pending()
        for _, packed in self.pending:
            packed.release()
        for f in self.files.values():
            if f.writer is not None:
                f.writer.abort()
                f.writer = None
        self.summary["fallback_batches"] = getattr(self.dec, "fallback_batches", 0) - self.fb0
        self.summary["skipped_files"] = len(self.tok.skipped_files)
        self.log.finish()
        self.log.timings["bytes_downloaded"] = self.backend.bytes_downloaded


def decode_files(tok, inputs: Sequence[Tuple[str, str]], batch_size: int, chunk_size, num_workers: int, rescale: bool, device_writer: bool,
                 max_held_bytes: int, sample_rate: int, token_rate: int, audio_format: str = "wav", stream: bool = False, log: Optional[RunLog] = None) -> None:
    """The loop of ``AudioToken.decode_batch_files`` (``DecodeRun``)."""
    DecodeRun(tok, inputs, batch_size, chunk_size, num_workers, rescale, device_writer, max_held_bytes, sample_rate, token_rate, audio_format, stream, log).run()
