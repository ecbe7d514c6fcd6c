"""What the whole-file runs share (``encode_batch_files``: encode_files.py, ``decode_batch_files``: decode_files.py, ``fit_quantizer``): the run log — who was
skipped, the per-stage host seconds, the final report — and the steps every driver takes the same way: listing and sharding the inputs, building the device
feeder, taking a feeder batch over onto the compute stream, appending a row's tokens to its file."""
from __future__ import annotations

import os
import time
from typing import List

import torch

from .configs import AUDIO_EXTS, TAR_EXTS, ZIP_EXTS
from .harness import save_audio_tokens, save_rel_audio_tokens
from .logger import get_logger

logger = get_logger(__name__, log_file=None, level="WARNING")


class RunLog:
    """The record of ONE file run over ``tok`` (an ``AudioToken``): ``what`` is the public method's name, ``product`` ("token" / "audio") the kind of file a
    skipped input does not get. ``timings`` are host seconds per stage of the loop — `stage` = producing the next batch (decode wait, validation, padding,
    upload), `encode_call` = enqueueing the model call, `device_wait` = blocked on the device (the status read of ``verified``, the first ``.cpu()``, the
    peaks), `save` = writing the batch BEFORE while the device works on the current one — plus the batches / rows counters; a driver publishes them as
    ``tok.run_timings``."""
    STAGES = ("stage_s", "encode_call_s", "device_wait_s", "save_s")

    def __init__(self, tok, what: str, product: str = "token"):
        self.tok, self.what, self.product = tok, what, product
        self.start_time = time.time()
        self.timings = {"stage_s": 0.0, "encode_call_s": 0.0, "device_wait_s": 0.0, "save_s": 0.0, "batches": 0, "rows": 0}

    def skipped(self, name, why) -> None:
        """An input the run cannot use (undecodable, invalid, dropped): recorded in ``tok.skipped_files``, and the run goes on."""
        logger.error(f"Skipping {name}: {why}")
        self.tok.skipped_files.append((name, why))

    def laps(self, keys, *times) -> None:
        """``times`` = ``len(keys) + 1`` readings of ``time.perf_counter()`` in order: the interval between two neighbours goes to the key at that place."""
        for key, a, b in zip(keys, times, times[1:]):
            self.timings[key] += b - a

    def lap(self, key: str, since: float) -> None:
        self.timings[key] += time.perf_counter() - since

    def batch(self, rows: int) -> None:
        self.timings["batches"] += 1
        self.timings["rows"] += rows

    def guard(self, doing: str) -> "_Guard":
        """``with log.guard("... failed"):`` around the bookkeeping in a ``finally``: an ``Exception`` in the block is logged and swallowed, so it cannot mask
        the exception that ended the run (which passes the ``finally`` untouched)."""
        return _Guard(f"{self.what}: {doing}")

    def finish(self) -> None:
        self.timings["total_s"] = time.time() - self.start_time

    def report(self) -> None:
        skipped = self.tok.skipped_files
        if skipped:
            logger.error(f"{self.what}: {len(skipped)} input(s) were skipped and have NO {self.product} file (AudioToken.skipped_files): "
                         + "; ".join(f"{p} ({why})" for p, why in skipped[:8]) + (" ..." if len(skipped) > 8 else ""))


class _Guard:
    def __init__(self, prefix: str):
        self.prefix = prefix

    def __enter__(self):
        return self

    def __exit__(self, kind, e, tb) -> bool:
        if kind is None or not issubclass(kind, Exception):
            return False
        logger.error(f"{self.prefix}: {kind.__name__}: {e}")
        return True


# ---- the inputs -------------------------------------------------------------------------------------------------------------------------------------------------
def input_files(audio_files, audio_dir, exts=None) -> List[str]:
    """The inputs of encode_batch_files / fit_quantizer / decode_batch_files: the given files, or every file with a known extension (``exts``; default: the
    audio and archive extensions) under ``audio_dir``, sorted."""
    if audio_files is not None:
        return [str(f) for f in audio_files]
    # every file under audio_dir with one of the extensions — the set the reference's `glob.iglob(f"{audio_dir}/**/*{ext}", recursive=True)` per
    # extension finds (datasets.py:47-50; glob does not descend into or match dot-names) — in ONE walk instead of fourteen, sorted (the sharding
    # needs every rank to see the same order)
    exts = tuple(exts) if exts is not None else AUDIO_EXTS + TAR_EXTS + ZIP_EXTS
    files = []
    seen = set()    # glob follows symlinked sub-directories (datasets laid out as symlink farms); so does this walk, once per real directory
    try:            # the root counts as seen: a link cycle back to it must not list its own files a second time
        st = os.stat(str(audio_dir))
        seen.add((st.st_dev, st.st_ino))
    except OSError:
        pass
    for d, dirs, names in os.walk(str(audio_dir), followlinks=True):
        keep = []
        for x in dirs:
            if x.startswith("."):
                continue
            try:
                st = os.stat(os.path.join(d, x))
            except OSError:
                continue
            if (st.st_dev, st.st_ino) not in seen:
                seen.add((st.st_dev, st.st_ino))
                keep.append(x)
        dirs[:] = keep
        files.extend(os.path.join(d, n) for n in names if n.endswith(exts) and not n.startswith("."))
    files.sort()
    return files


def shard_files(tok, files: List[str]) -> List[str]:
    """This rank's share of the file list under torch.distributed (collective: every rank calls it with the same list)."""
    import hashlib
    import torch.distributed as dist
    from .distributed import collective_device, gather_scalars, shard_by_size
    # duration-aware: whole files by greedy LPT on their sizes (distributed.shard_by_size). Rank 0 stats the list ONCE and broadcasts the sizes (N_files
    # stats instead of N_files x world on a shared filesystem; and every rank provably shards the same numbers)
    digest = hashlib.sha256("\0".join(files).encode("utf-8", "surrogateescape")).hexdigest()
    sizes = [([os.path.getsize(f) if os.path.exists(f) else 0 for f in files], digest)] if dist.get_rank() == 0 else [None]
    # the pickled list travels on THIS rank's device under RCCL (not torch's current device: a caller that never called set_device would put every rank on cuda:0)
    dist.broadcast_object_list(sizes, src=0, device=collective_device(torch.device(tok.device), dist))
    sizes, digest0 = sizes[0]
    # every rank learns whether ALL ranks hold rank 0's list: a rank that differs must stop the others too, not let them encode a shard of a list it does not share
    same = len(sizes) == len(files) and digest0 == digest
    votes = gather_scalars([1.0 if same else 0.0], torch.device(tok.device), dist)
    bad = [r for r, v in enumerate(votes) if v[0] != 1.0]
    assert not bad, f"ranks {bad} see a different file list than rank 0: encode_batch_files needs the same audio_files / audio_dir on every rank"
    return [files[i] for i in shard_by_size(sizes, dist.get_rank(), dist.get_world_size())]


def shard_if_distributed(tok, files: List[str], wanted: bool = True) -> List[str]:
    """``files``, or this rank's share of them when ``torch.distributed`` runs more than one rank and the caller has not switched the sharding off
    (``shard_across_ranks=False``)."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1 and wanted:
        return tok._shard_files(files)
    return files


# ---- steps of the loops ---------------------------------------------------------------------------------------------------------------------------------------
def new_feeder(tok, chunk_size, num_workers, skipped, transform):
    """The device feeder (feeder.py) for ``tok``'s model: its sample rate, token rate and pad token."""
    from .feeder import DeviceFeeder
    cfg = tok.model_config
    return DeviceFeeder(tok.device, cfg.model_sample_rate, chunk_size, cfg.model_token_rate, cfg.pad_token, num_workers, skipped, transform=transform)


def take_over(ev, device, *tensors) -> None:
    """A staged batch changes streams: ``device``'s current stream waits for the upload's event ``ev``, and the allocator learns that the tensors are in use
    there. ``ev`` None: the batch was not made on a side stream and there is nothing to wait for."""
    if ev is not None:
        stream = torch.cuda.current_stream(device)
        stream.wait_event(ev)
        for t in tensors:
            t.record_stream(stream)


def save_tokens(tokens, pointer, outdir, audio_files, audio_dir) -> None:
    """One row's trimmed tokens appended to its file: flat in ``outdir`` for a file list, at the mirrored relative path for a directory."""
    if audio_files is not None:
        save_audio_tokens(tokens, pointer, str(outdir))
    else:
        save_rel_audio_tokens(tokens, pointer, str(outdir), str(audio_dir))
