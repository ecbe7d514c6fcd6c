"""The run behind ``AudioToken.to_audio_batch_files``: semantic token files -> audio files. It is ``decode_files.DecodeRun`` with another
source of tokens: ``valid_files()`` reads the next ``round_files`` valid sources, runs them through the GPT's generation queue (``to_acoustic(long_form=True,
slots=)``, §20) and the fine stage's window queue (``to_fine(slots=)``, §21), and hands each file's ``[8, T]`` codes to the planners as if it had been read
from an acoustic token file. Everything after that — the batches or stream ticks, the decoder at 8 code books, ``verified``, hold / rescale, the device PCM
and FLAC writers, the removal of half-written files — is the existing decode run. The planners pull lazily, so a round is generated when the decode side
needs it, and only one round's ids and one decode batch's audio are ever held.

The draws of a file come from ``file_draws``: a Philox stream keyed by the run's seed and the file's relative output stem, so that they do not depend on
what else is in the directory, on the round size or on the ranks."""
from __future__ import annotations

import os
import time
from typing import List, Optional, Sequence, Tuple

import numpy as np

from .decode_files import DecodeRun, _File
from .fine_decoder import MAX_QUEUE_ROWS, N_PASSES, fine_windows, history_cells
from .prefetch import ordered_map
from .runs import RunLog
from .semantic_decoder import MAX_SOURCE_IDS, acoustic_windows, check_windows, default_window, stream_extent
from .writer import TokenFileError

NO_FRAME = "stage 1 produced no whole frame of coarse codes"


def fnv1a64(text: str) -> int:
    """The 64-bit FNV-1a hash of ``text``'s UTF-8 bytes."""
    h = 0xCBF29CE484222325
    for byte in text.encode("utf-8", "surrogateescape"):
        h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def file_draws(seed: int, stem: str, gpt_capacity: int, n_windows: int = 0, block: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """The draws of one file: ``(gpt, fine)`` from ``np.random.Generator(np.random.Philox(key=[seed, fnv1a64(stem)]))``, ``stem`` being the file's output
    path relative to ``outdir`` without its extension, in posix form. First ``gpt``: float32 ``[gpt_capacity]``, one draw per position of the source's own
    stage 1 stream (``semantic_decoder.stream_extent`` of the source alone); then ``fine``: float32 ``[n_windows, 6, block]``, the fine stage's draws for
    the frames stage 1 produced. Asking for no fine draws (``n_windows = 0``) gives the same ``gpt``."""
    g = np.random.Generator(np.random.Philox(key=[int(seed), fnv1a64(stem)]))
    gpt = g.random(int(gpt_capacity), dtype=np.float32)
    return gpt, g.random((int(n_windows), N_PASSES, int(block)), dtype=np.float32)


def stack_gpt_draws(draws: Sequence[np.ndarray], L: Optional[int] = None) -> np.ndarray:
    """Per-file stage 1 draws -> the ``[B, L]`` array ``to_acoustic(long_form=True)`` takes: zero-padded to ``L`` (default: the longest); positions past a
    row's own capacity are never read."""
    L = max(len(d) for d in draws) if L is None else int(L)
    out = np.zeros((len(draws), L), dtype=np.float32)
    for b, d in enumerate(draws):
        out[b, :len(d)] = d
    return out


def output_stem(out: str, outdir: str) -> str:
    """The key of a file's draws: its output path relative to ``outdir``, without the extension, in posix form."""
    return os.path.splitext(os.path.relpath(out, start=str(outdir)))[0].replace(os.sep, "/")


def read_semantic_file(path, vocab: int, max_ids: int = MAX_SOURCE_IDS) -> np.ndarray:
    """The int64 ``[T]`` semantic ids of a token file (int16 or int64 ``[T]``, ``[1, T]`` or ``[1, 1, T]``), validated on the host."""
    try:
        arr = np.load(str(path), allow_pickle=False)
    except Exception as e:   # noqa: BLE001 — np.load raises ValueError / OSError / EOFError / UnpicklingError depending on how the file is damaged
        raise TokenFileError(f"unreadable token file ({type(e).__name__}: {e})") from e
    if not isinstance(arr, np.ndarray):
        raise TokenFileError("unreadable token file (not a single .npy array)")
    if arr.dtype not in (np.dtype(np.int16), np.dtype(np.int64)):
        raise TokenFileError(f"token dtype {arr.dtype} (int16 or int64 expected)")
    if not (1 <= arr.ndim <= 3) or any(d != 1 for d in arr.shape[:-1]):
        raise TokenFileError(f"token array of rank {arr.ndim} with shape {tuple(arr.shape)} ([T], [1, T] or [1, 1, T] expected)")
    arr = arr.reshape(-1).astype(np.int64)
    if arr.size == 0:
        raise TokenFileError("empty token file (T = 0)")
    if arr.size > max_ids:
        raise TokenFileError(f"{arr.size} semantic ids, more than the {max_ids} one source may have")
    lo, hi = int(arr.min()), int(arr.max())
    if lo < 0 or hi >= vocab:
        raise TokenFileError(f"semantic id {lo if lo < 0 else hi} outside [0, {vocab - 1}]")
    return arr


class SemanticRun(DecodeRun):
    """One ``to_audio_batch_files`` call. ``inputs`` = (token file, output path) in order; ``stages`` turns one round of sources into codes: a callable
    ``(sources, stems) -> (codes, info)`` with ``codes[b]`` int64 ``[8, T_b]`` or None (stage 1 produced no whole frame) — ``Stages`` below on a device,
    a stub in the tests that need none."""

    def __init__(self, tok, decoder, inputs, outdir, stages, vocab: int, round_files: int, codes_dir, *args, **kwargs):
        super().__init__(tok, inputs, *args, decoder=decoder, **kwargs)
        self.outdir, self.stages, self.vocab, self.round_files, self.codes_dir = str(outdir), stages, int(vocab), int(round_files), codes_dir
        self.summary.update({"rounds": 0, "gpt_ticks": 0, "fine_passes": 0, "generated_frames": 0})
        self.log.timings.update({"gpt_s": 0.0, "fine_s": 0.0})

    def load(self, item):
        i, (path, out) = item
        try:
            return i, path, out, read_semantic_file(path, self.vocab, MAX_SOURCE_IDS - len(getattr(self.stages, "voice", None) or ())), None
        except TokenFileError as e:
            return i, path, out, None, str(e)

    def rounds(self):
        """Lists of up to ``round_files`` valid (input index, path, output, ids), ``num_workers`` files read ahead, in order; the others are skipped."""
        this: List[tuple] = []
        for i, path, out, ids, why in ordered_map(self.load, list(enumerate(self.inputs)), self.num_workers):
            if ids is None:
                self.log.skipped(path, why)
                continue
            this.append((i, path, out, ids))
            if len(this) == self.round_files:
                yield this
                this = []
        if this:
            yield this

    def valid_files(self):
        """(input index, 8, T) of every file whose round has been generated, in order."""
        for members in self.rounds():
            stems = [output_stem(out, self.outdir) for _, _, out, _ in members]
            codes, info = self.stages([ids for _, _, _, ids in members], stems)
            self.summary["rounds"] += 1
            for key in ("gpt_ticks", "fine_passes"):
                self.summary[key] += int(info.get(key, 0))
            for key in ("gpt_s", "fine_s"):
                self.log.timings[key] += float(info.get(key, 0.0))
            for (i, path, out, _), stem, c in zip(members, stems, codes):
                if c is None:
                    self.log.skipped(path, NO_FRAME)
                    continue
                c = np.ascontiguousarray(np.asarray(c), dtype=np.int64)
                K, T = c.shape
                if self.codes_dir is not None:
                    try:
                        dst = os.path.join(str(self.codes_dir), *stem.split("/")) + ".npy"
                        os.makedirs(os.path.dirname(dst), exist_ok=True)
                        np.save(dst, c.astype(np.int16))
                    except OSError as e:
                        self.log.skipped(path, f"cannot write its codes: {type(e).__name__}: {e}")
                        continue
                self.summary["generated_frames"] += T
                step = self.chunk_frames
                self.files[i] = _File(path, out, c, rows_left=1 if step is None else (T + step - 1) // step)
                yield i, K, T


class Stages:
    """One round through the two generators of ``tok`` (a semantic ``AudioToken``): the GPT's generation queue with each file's own draws, then the fine
    stage's window queue, its rows handed over longest first to cut the tail (rows are independent of each other, so the order changes no result)."""

    def __init__(self, tok, seed: int, temperature: float, top_k: int, fine_temperature, max_new_tokens: int, window, hop, slots: int, fine_slots: int,
                 voice=None, top_p=None, min_p=None):
        self.voice = voice         # one VoicePrompt that every file continues, or None
        self.top_p, self.min_p = top_p, min_p   # stage 1's truncation after the top-k, None: off
        self.tok, self.seed, self.temperature, self.top_k, self.fine_temperature = tok, int(seed), temperature, top_k, fine_temperature
        self.max_new, self.slots, self.fine_slots = int(max_new_tokens), int(slots), int(fine_slots)
        gpt = tok._gpt()
        cfg = gpt.config
        self.r, self.block = int(cfg.ids_per_source_token), gpt.block_size
        self.S = default_window(cfg, self.block)[0] if window is None else int(window)
        self.H = (self.S // 2) // 2 * 2 if hop is None else int(hop)
        check_windows(self.S, self.H, self.r, self.block)   # a bad window / hop is refused before any file is read
        if not 1 <= self.max_new <= 1024:
            raise ValueError(f"to_audio_batch_files: max_new_tokens must be 1 to 1024, got {self.max_new}")
        self.W = tok._fine().block_size
        if voice is not None:      # a prompt that no source can follow is refused before any file is read
            from .semantic_decoder import check_prompt
            from .voice import VoicePrompt
            if not isinstance(voice, VoicePrompt) or voice.codes.shape[0] != 8:
                raise ValueError("to_audio_batch_files: voice must be one VoicePrompt with all 8 code books")
            check_prompt(len(voice), 1, self.S, self.H)
        self.last_coarse = None    # the last round's AcousticGeneration (tests)

    def capacity(self, n_ids: int) -> int:
        """The positions of a source's own stage 1 stream."""
        P = len(self.voice) if self.voice is not None else 0
        return stream_extent([acoustic_windows(n_ids, self.S, self.H, self.r, self.block, P)], self.S, self.r, self.max_new, self.block, [P])[1]

    def __call__(self, sources, stems):
        tok, W = self.tok, self.W
        caps = [self.capacity(len(s)) for s in sources]
        t0 = time.perf_counter()
        u = stack_gpt_draws([file_draws(self.seed, stem, cap)[0] for stem, cap in zip(stems, caps)])
        coarse = tok.to_acoustic(list(sources), max_new_tokens=self.max_new, temperature=self.temperature, top_k=self.top_k, uniforms=u, long_form=True,
                                 window=self.S, hop=self.H, slots=self.slots, voice=self.voice, top_p=self.top_p, min_p=self.min_p)
        self.last_coarse = coarse
        t1 = time.perf_counter()
        have = [b for b, c in enumerate(coarse.codes) if c is not None and c.shape[1] >= 1]
        order = sorted(have, key=lambda b: -int(coarse.codes[b].shape[1]))   # longest first; equal lengths stay in file order
        codes: List[Optional[np.ndarray]] = [None] * len(sources)
        info = {"gpt_ticks": len(coarse.ticks or ()), "fine_passes": 0, "gpt_s": t1 - t0, "fine_s": 0.0}
        if order:
            draws = None
            if self.fine_temperature is not None:
                h = history_cells(self.voice.frames, W) if self.voice is not None else 0
                draws = [file_draws(self.seed, stems[b], caps[b], len(fine_windows(int(coarse.codes[b].shape[1]), W, h)), W)[1] for b in order]
            fine = tok.to_fine([coarse.codes[b] for b in order], temperature=self.fine_temperature, uniforms=draws, slots=self.fine_slots,
                               history=None if self.voice is None else self.voice.codes)
            for b, c in zip(order, fine.codes):
                codes[b] = c.numpy()
            info["fine_passes"] = len(fine.passes)
            info["fine_s"] = time.perf_counter() - t1
        return codes, info


def to_audio_files(tok, decoder, inputs, outdir, stages, vocab, round_files, codes_dir, batch_size, chunk_size, num_workers, rescale, device_writer,
                   max_held_bytes, sample_rate, token_rate, audio_format="wav", stream=False, log: Optional[RunLog] = None) -> None:
    """The loop of ``AudioToken.to_audio_batch_files`` (``SemanticRun``)."""
    if not 1 <= int(round_files) <= MAX_QUEUE_ROWS:
        raise ValueError(f"to_audio_batch_files: round_files must be 1 to {MAX_QUEUE_ROWS}, got {round_files}")
    SemanticRun(tok, decoder, inputs, outdir, stages, vocab, round_files, codes_dir, batch_size, chunk_size, num_workers, rescale, device_writer,
                max_held_bytes, sample_rate, token_rate, audio_format, stream, log).run()
