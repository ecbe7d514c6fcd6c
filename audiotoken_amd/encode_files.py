"""The loops behind ``AudioToken.encode_batch_files`` and the frame collection of ``AudioToken.fit_quantizer``: the host chunk stream (``ChunkStream``), the
chunked run (``ChunkedEncode``: one clip per ``chunk_size``-second segment), the streamed run (``StreamedEncode``: one clip per file) and
``collect_frames``. Every run writes its skips, timings and final report through one ``runs.RunLog``; the façade (core.py) checks the arguments, lists the
files and delegates.

The speed of a run is its overlap, so the ORDER of the steps in ``run`` is part of each driver's contract and is stated in its docstring."""
from __future__ import annotations

import time
from collections import deque

import numpy as np
import torch

from . import prng
from .audio_io import AudioDecodeError, iterate_tar, iterate_zip, process_audio_chunks
from .configs import AUDIO_EXTS, TAR_EXTS, ZIP_EXTS, AudioConfig
from .harness import batched, collate_fn, iter_chunk
from .logger import get_logger
from .prefetch import background, ordered_map
from .runs import RunLog, new_feeder, save_tokens, take_over
from .writer import plan_encode_stream_ticks

logger = get_logger(__name__, log_file=None, level="WARNING")


def in_flight(start, items, depth):
    """``start(item)`` for up to ``depth`` items ahead of the consumer, results in order (``start`` returns immediately: it submits work elsewhere)."""
    pending = deque()
    for it in items:
        pending.append(start(it))
        if len(pending) >= max(1, depth):
            yield pending.popleft()
    while pending:
        yield pending.popleft()


class ChunkStream:
    """File -> streamed ``chunk_size``-second chunks -> segments (reference datasets.py:107-139). Decoding and resampling run ``num_workers`` files
    ahead of the consumer — in SPAWNED worker processes for plain audio files when ``worker_processes`` (the reference's DataLoader workers,
    core.py:259-267; the parent has the GPU initialised, so never forked), else on a thread pool; archives are streamed member by member by a
    background thread either way (members are not random-access). The segment order equals the sequential one."""

    def __init__(self, tok, skipped, chunk_size: int, num_workers: int = 0, worker_processes: bool = False):
        self.tok, self.skipped, self.chunk_size, self.num_workers = tok, skipped, chunk_size, num_workers
        self.sr = tok.model_config.model_sample_rate
        self.worker_processes = bool(worker_processes) and num_workers > 0
        self.pool = None       # the worker processes: started by `segments`, with its first segment

    def load(self, file_path: str):
        """One unit of host work: plain audio files are decoded completely; archives return a streaming source. A file that
        cannot be decoded (AudioDecodeError: a codec this build does not ship, more than one channel, a damaged header) is skipped, recorded
        in ``tok.skipped_files`` and reported at the end of the run — it must not abort a run whose earlier files have already been
        appended to. Any other exception propagates, as in the reference (datasets.py __iter__)."""
        sr, chunk_size, skipped = self.sr, self.chunk_size, self.skipped
        if file_path.endswith(AUDIO_EXTS):
            if self.pool is not None:
                from ._workers import decode_chunks
                return self.pool.submit(decode_chunks, file_path, sr, chunk_size)
            try:
                return list(process_audio_chunks(file_path, sr, chunk_size))
            except AudioDecodeError as e:
                skipped(file_path, str(e))
                return []
        if file_path.endswith(TAR_EXTS):
            return background(lambda: iterate_tar(file_path, sr, chunk_size, skipped)) if self.num_workers > 0 else iterate_tar(file_path, sr, chunk_size, skipped)
        if file_path.endswith(ZIP_EXTS):
            return background(lambda: iterate_zip(file_path, sr, chunk_size, skipped)) if self.num_workers > 0 else iterate_zip(file_path, sr, chunk_size, skipped)
        logger.error(f"File {file_path} not supported for processing. Only {AUDIO_EXTS + TAR_EXTS + ZIP_EXTS} supported")
        self.tok.skipped_files.append((file_path, "unsupported extension"))
        return []

    def resolve(self, file_path, source):
        if self.pool is not None and hasattr(source, "result"):      # a worker process's answer: numpy chunks, or the reason the file was skipped
            kind, payload = source.result()
            if kind == "skip":
                self.skipped(file_path, payload)
                return []
            return [(torch.from_numpy(c), file_path) for c in payload]
        return source

    def segments(self, files):
        cfg = self.tok.model_config
        names = [str(f) for f in files]
        start = lambda f: (f, self.load(f))
        if self.worker_processes:
            import multiprocessing as mp
            from concurrent.futures import ProcessPoolExecutor
            self.pool = ProcessPoolExecutor(max_workers=self.num_workers, mp_context=mp.get_context("spawn"))
        try:
            # with processes `load` only SUBMITS (the thread pool of ordered_map is not needed: in-line submission keeps num_workers futures in flight)
            sources = ordered_map(start, names, self.num_workers) if self.pool is None else in_flight(start, names, self.num_workers)
            for file_path, source in sources:
                source = self.resolve(file_path, source)
                try:
                    for waveform, file_name in source:
                        yield from iter_chunk(waveform, file_name, sample_rate=cfg.model_sample_rate, chunk_size=self.chunk_size,
                                              model_token_rate=cfg.model_token_rate, pad_token=cfg.pad_token, transform=self.tok.transform_func)
                finally:   # an exception in the consumer (or an abandoned run) must not leave an archive's producer thread and its handle behind
                    close = getattr(source, "close", None)
                    if close is not None:
                        close()
        finally:
            if self.pool is not None:
                self.pool.shutdown(wait=False, cancel_futures=True)


def end_of_run(tok) -> None:
    """End of an encode_batch_files run: layers the range fallback moved to bf16x3 because of THIS run's inputs go back to f16x2 (a loud or clipped file
    must not slow down, or change the rounding of, every later run of the process); what happened is kept in ``run_summary``."""
    enc = tok.encoder
    tok.run_summary = {"fallback_batches": getattr(enc, "fallback_batches", 0), "pinned_layers": sorted(set(getattr(enc, "pinned_layers", []) or [])),
                       "nonfinite_batches": getattr(enc, "nonfinite_batches", 0), "skipped_files": len(tok.skipped_files)}
    if tok.run_summary["pinned_layers"]:
        logger.error(f"encode_batch_files: layers {tok.run_summary['pinned_layers']} ran on bf16x3 for part of this run (fp16 range overflow); restored to f16x2")
    if hasattr(enc, "unpin_layers"):
        enc.unpin_layers()


# ---- the chunked run ------------------------------------------------------------------------------------------------------------------------------------------
class ChunkedEncode:
    """``encode_batch_files`` without ``stream``. Per batch k, in this order: ENQUEUE its encode (asynchronous on the device); SAVE batch k - 1 (its tokens
    came to the host one iteration ago; ownership is taken before the save); STAGE batch k + 1 (decoded / uploaded / cut while k encodes); COLLECT k —
    ``verified``, then ONE device-to-host copy. The save is deferred by one batch and is not lost by it: ``run`` writes the pending batch also when the
    encode or the staging of the next one raised."""
    LAPS = ("encode_call_s", "save_s", "stage_s", "device_wait_s")     # the intervals of one iteration, in the order of its steps

    def __init__(self, tok, log: RunLog, files, batch_size, outdir, chunk_size, num_workers, audio_files, audio_dir, options):
        self.tok, self.log, self.outdir, self.audio_files, self.audio_dir = tok, log, outdir, audio_files, audio_dir
        self.on_gpu = torch.device(tok.device).type == "cuda"
        self.copy_stream = torch.cuda.Stream(device=tok.device) if self.on_gpu else None
        self.pending = None    # (tokens on the host, file pointers) of the batch before: written while the device encodes the next one, in batch order
        # Device feeder (feeder.py): decoding stays on the host, sample conversion / per-chunk resampling / segmentation / padding run in one HIP kernel per
        # batch — for semantic_s including its per-chunk zero-mean / unit-variance transform (feeder.py, transform="zmuv"); a custom transform_func and
        # `device_feeder=False` keep the host data flow of the reference.
        from .hubert import hubert_processor as _zmuv
        dev_transform = "zmuv" if tok.transform_func is _zmuv else None     # semantic_s: the per-chunk normalisation runs in the feeder's kernels
        tok.feeder_timings = None
        if self.on_gpu and (tok.transform_func is None or dev_transform) and options.get("device_feeder", True):
            feeder = new_feeder(tok, chunk_size, num_workers, log.skipped, dev_transform)
            tok.feeder_timings = feeder.timings
            self.staged = feeder.batches(files, batch_size)
        else:
            chunks = ChunkStream(tok, log.skipped, chunk_size, num_workers, bool(options.get("worker_processes", False)))
            self.staged = (self.upload(b) for b in batched(chunks.segments(files), batch_size))

    def upload(self, batch):
        """Collate a batch and start its host->device copy (pinned staging, side stream) so it overlaps the encode of
        the batch before it; returns (ids, masks, file_pointers, ready_event)."""
        device = self.tok.device
        input_ids, attention_masks, file_pointers = collate_fn(batch)
        if not self.on_gpu:
            return input_ids.to(device), attention_masks.to(device), file_pointers, None
        with torch.cuda.stream(self.copy_stream):
            ids = input_ids.pin_memory().to(device, non_blocking=True)
            masks = attention_masks.pin_memory().to(device, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(self.copy_stream)
        return ids, masks, file_pointers, ev

    def stage_next(self):
        """The next (ids, masks, file_pointers, ready_event), or None: the decode wait + upload + descriptors of the feeder, or the host chunk stream +
        collate + upload."""
        return next(self.staged, None)

    def enqueue(self, staged):
        input_ids, attention_masks, _, ev = staged
        take_over(ev, self.tok.device, input_ids, attention_masks)
        return self.tok.encoder(input_ids, attention_masks)      # asynchronous on the device

    def save_pending(self) -> None:
        """The per-row trim + append to the .npy files of the batch before."""
        if self.pending is not None:
            p, self.pending = self.pending, None      # ownership first: an interrupt inside the save must not make the `finally` of `run` append the rows again
            for tokens, pointer in zip(*p):
                save_tokens(tokens, pointer, self.outdir, self.audio_files, self.audio_dir)

    def collect(self, encoded, staged) -> None:
        input_ids, attention_masks, file_pointers, _ = staged
        enc = self.tok.encoder
        if hasattr(enc, "verified"):   # the copy below synchronises anyway: check the call's device status first
            encoded = enc.verified(encoded, input_ids, attention_masks)
        self.pending = (encoded.cpu(), file_pointers)   # ONE device-to-host copy per batch (a per-row .cpu() inside the save would synchronise B times)

    def run(self) -> None:
        log = self.log
        t0 = time.perf_counter()
        staged = self.stage_next()
        log.lap("stage_s", t0)
        try:
            while staged is not None:
                t0 = time.perf_counter()
                encoded = self.enqueue(staged)
                t1 = time.perf_counter()
                self.save_pending()
                t2 = time.perf_counter()
                nxt = self.stage_next()
                t3 = time.perf_counter()
                self.collect(encoded, staged)
                log.laps(self.LAPS, t0, t1, t2, t3, time.perf_counter())
                log.batch(len(staged[2]))
                staged = nxt
        finally:
            # also when the encode / staging of batch k raised: the verified tokens of batch k - 1 are on the host and belong in their files (earlier
            # batches are already there)
            if self.pending is not None:
                t0 = time.perf_counter()
                self.save_pending()
                log.lap("save_s", t0)
            with log.guard("end-of-run bookkeeping failed"):
                end_of_run(self.tok)
        log.finish()
        logger.debug(f"Encoding batch files took: {time.time() - log.start_time:.2f}s")
        log.report()


# ---- the streamed run -----------------------------------------------------------------------------------------------------------------------------------------
class StreamedEncode:
    """``encode_batch_files(stream=True)``: ticks over a stream pool (writer.plan_encode_stream_ticks). A tick, in this order: STAGE — the files that take
    the free slots are opened and every live file's next chunk is picked (``resample="file"``: a file's units are the ticks of its resident PCM,
    resample_stream.ResidentFiles, and the tick's chunks come out of ONE resample launch); PUSH them and flush the files whose chunks are exhausted (their
    slots go to the next files, in order); bring the tick's new frames TO the HOST in one copy; APPEND them to the token files and free the finished
    files. (There is no deferred save here: a tick's frames are on disk before the next tick starts.)"""
    LAPS = ("stage_s", "encode_call_s", "device_wait_s", "save_s")

    def __init__(self, tok, log: RunLog, files, batch_size: int, outdir, chunk_size, num_workers: int, audio_files, audio_dir, resample: str = "chunk",
                 max_file_bytes: int = 4 << 30):
        self.tok, self.log, self.files, self.batch_size = tok, log, files, batch_size
        self.outdir, self.chunk_size, self.num_workers, self.audio_files, self.audio_dir = outdir, chunk_size, num_workers, audio_files, audio_dir
        self.sr, self.rate = tok.model_config.model_sample_rate, tok.model_config.model_token_rate
        tok.feeder_timings = None
        self.opened: list = []     # position in the tick plan -> [path, chunks]
        self.sids: dict = {}       # position in the tick plan -> stream id, while the file is live
        self.resident = None
        if resample == "file":
            from .resample_stream import ResidentFiles
            self.resident = ResidentFiles(tok.device, self.sr, chunk_size, num_workers, log.skipped, max_file_bytes=max_file_bytes, min_samples=321)
        self.pool = tok.encoder.new_stream_pool(batch_size)

    def load(self, path: str):
        """One file's chunks, decoded ``num_workers`` files ahead: (path, [samples [n] per chunk] or None, reason)."""
        if not path.endswith(AUDIO_EXTS):
            return path, None, ("stream=True takes plain audio files: archives are not streamed" if path.endswith(TAR_EXTS + ZIP_EXTS)
                                else "unsupported extension")
        try:
            return path, [chunk[0] for chunk, _ in process_audio_chunks(path, self.sr, self.chunk_size)], None
        except AudioDecodeError as e:
            return path, None, str(e)

    def chunk_counts(self):
        """What the tick plan reads: per usable file, in order, its chunks (only their number counts); the file is entered in ``opened`` on the way."""
        if self.resident is not None:
            for f in self.resident.open_all(self.files):    # [name, the file on the device]: its PCM is released with this entry, after its flush
                self.opened.append([f.name, f])
                yield range(f.ticks)
            return
        for path, chunks, why in ordered_map(self.load, [str(f) for f in self.files], self.num_workers):
            if chunks is None:
                self.log.skipped(path, why)
            elif sum(int(c.shape[-1]) for c in chunks) < 321:   # the library's rule for a clip (a stream whose first push is its last is a one-shot encode)
                self.log.skipped(path, "fewer than 321 samples")
            else:
                self.opened.append([path, chunks])
                yield [int(c.shape[-1]) for c in chunks]

    def stage(self, tick) -> dict:
        """{stream id: samples} of the tick; a file on its first tick gets its slot here."""
        opened, sids, resident, feed = self.opened, self.sids, self.resident, {}
        for r in tick:
            if r.file not in sids:
                sids[r.file] = self.pool.open()
            if resident is None:
                chunks = opened[r.file][1]
                feed[sids[r.file]], chunks[r.t0] = chunks[r.t0], None
        if resident is not None:
            for r, x in zip(tick, resident.chunks([(opened[r.file][1], r.t0) for r in tick])):
                feed[sids[r.file]] = x
        return feed

    def push(self, tick, feed):
        """(new frames per stream id, the last frames of the files that end with this tick, those files)."""
        out = self.pool.push(feed)           # every group's status word is read in there: the tokens are verified when it returns
        last = [r.file for r in tick if r.last]
        fin = self.pool.flush([self.sids[i] for i in last]) if last else {}
        return out, fin, last

    def to_host(self, tick, out, fin):
        parts = []
        for r in tick:
            sid = self.sids[r.file]
            parts.append(torch.cat([out[sid], fin[sid]], dim=-1) if sid in fin else out[sid])
        return parts, torch.cat(parts, dim=-1).cpu()   # ONE device-to-host copy per tick

    def append(self, tick, parts, host, last) -> None:
        pos = 0
        for r, p in zip(tick, parts):
            t = p.shape[-1]
            if t:
                path, codes = self.opened[r.file][0], host[:, pos:pos + t]
                pointer = AudioConfig(file_name=path, length_seconds=codes.shape[-1] / self.rate, model_token_rate=self.rate)
                save_tokens(codes, pointer, self.outdir, self.audio_files, self.audio_dir)
            pos += t
        for i in last:
            del self.sids[i]
            self.opened[i] = None

    def run(self) -> None:
        tok, log = self.tok, self.log
        try:
            ticks = plan_encode_stream_ticks(self.chunk_counts(), self.batch_size)
            while True:
                t0 = time.perf_counter()
                tick = next(ticks, None)        # opens (waits for) the files that take the free slots
                if tick is None:
                    break
                feed = self.stage(tick)
                t1 = time.perf_counter()
                out, fin, last = self.push(tick, feed)
                t2 = time.perf_counter()
                parts, host = self.to_host(tick, out, fin)
                t3 = time.perf_counter()
                self.append(tick, parts, host, last)
                log.laps(self.LAPS, t0, t1, t2, t3, time.perf_counter())
                log.batch(len(tick))
        finally:
            with log.guard("end-of-run bookkeeping failed"):
                end_of_run(tok)
                tok.run_summary["library_pushes"] = self.pool.library_pushes
                if self.resident is not None:
                    tok.run_summary["resample_launches"] = self.resident.resampler.launches
                    self.resident.finish()
        log.finish()
        log.report()


def encode_files(tok, files, batch_size, outdir, chunk_size, num_workers, audio_files, audio_dir, stream: bool, resample: str, options) -> None:
    """The run of ``AudioToken.encode_batch_files`` over ``files`` (listed and sharded by the caller); ``options`` = its extra keyword arguments."""
    log = RunLog(tok, "encode_batch_files", "token")
    tok.run_timings = log.timings
    if stream:
        StreamedEncode(tok, log, files, int(batch_size), outdir, chunk_size, int(num_workers), audio_files, audio_dir, resample,
                       options.get("max_file_bytes", 4 << 30)).run()
    else:
        ChunkedEncode(tok, log, files, batch_size, outdir, chunk_size, num_workers, audio_files, audio_dir, options).run()


# ---- fit_quantizer's sample ---------------------------------------------------------------------------------------------------------------------------------------
def kept_frames(pointers, T: int, keep_fraction: float, seed: int):
    """(indices into the batch's ``[B * T]`` frames that enter the sample, valid frames seen): each row's valid frames (``length_tokens``), thinned by a
    counter-based draw keyed on (file, segment, frame) when ``keep_fraction`` < 1."""
    keep, seen = [], 0
    for b, p in enumerate(pointers):
        n_valid = min(T, int(p.length_tokens))
        seen += n_valid
        idx = np.arange(n_valid, dtype=np.int64)
        if keep_fraction < 1.0:
            u = prng.uniform01(f"fit_quantizer|{p.file_name}|{int(getattr(p, 'start_idx', 0))}", n_valid, seed)
            idx = idx[u < np.float32(keep_fraction)]
        keep.append(b * T + idx)
    return (np.concatenate(keep) if keep else np.zeros(0, np.int64)), seen


def collect_frames(tok, log: RunLog, enc, files, chunk_size, batch_size, num_workers, max_frames: int, d: int, split_ln: int, keep_fraction: float, seed: int):
    """The sample ``fit_quantizer`` fits on: ``files`` through the device feeder and ``enc`` (the tokenizer's encoder with ``quantize=False``), every batch
    checked by ``verified`` before it adds frames, normalised by the quantiser step's own LayerNorm kernel, in file / segment / frame order, at most
    ``max_frames``. Returns (frames ``[n, d]`` on the device, {"frames", "frames_seen", "batches", "truncated"})."""
    from . import _cabi
    from .hubert import hubert_processor
    from .configs import Tokenizers
    lib = _cabi.load()
    dev = torch.device(tok.device)
    transform = "zmuv" if tok.tokenizer_name == Tokenizers.semantic_s else None
    assert tok.tokenizer_name != Tokenizers.semantic_s or tok.transform_func in (None, hubert_processor)
    feeder = new_feeder(tok, chunk_size, num_workers, log.skipped, transform)
    frames = torch.empty((max_frames, d), dtype=torch.float32, device=dev)
    filled, truncated, batches, seen = 0, False, 0, 0
    for input_ids, masks, pointers, ev in feeder.batches(files, batch_size):
        take_over(ev, dev, input_ids, masks)
        hidden = enc(input_ids, masks)
        hidden = enc.verified(hidden, input_ids, masks)      # an fp16 range overflow: the batch is re-encoded before any frame is taken
        batches += 1
        B, T, _ = hidden.shape
        rows = hidden.reshape(B * T, d)
        y = torch.empty_like(rows)
        ws = torch.empty(((B * T + 7) // 8 * 8) * d * 4 if split_ln else 1, dtype=torch.uint8, device=dev)
        _cabi.check(lib.at_kmeans_layernorm(rows.data_ptr(), y.data_ptr(), B * T, d, split_ln, ws.data_ptr(), ws.numel(),
                                            _cabi.current_stream_handle(dev)), "at_kmeans_layernorm")
        sel, n_valid = kept_frames(pointers, T, keep_fraction, seed)
        seen += n_valid
        if filled + len(sel) > max_frames:
            sel = sel[:max_frames - filled]
            truncated = True
        if len(sel):
            frames[filled:filled + len(sel)] = y[torch.from_numpy(sel).to(dev)]
            filled += len(sel)
        if truncated:
            break
    return frames[:filled], {"frames": filled, "frames_seen": seen, "batches": batches, "truncated": truncated}
