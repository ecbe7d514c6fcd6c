"""``AudioToken`` — the reference's public façade (audiotoken/core.py:27-359) over the MI355X HIP library.

Same constructor, attributes, method signatures, return shapes/dtypes and exception types; the differences are
forced by the environment and stated here:
* ``device`` must be a HIP device (``"cuda[:i]"`` under PyTorch-ROCm). The reference's ``device="cpu"`` default
  would need a CPU path, which this package deliberately does not have — constructing with "cpu" raises
  ``ValueError`` at ``load_encoder`` time.
* checkpoints cannot be downloaded (no network): pass ``weights=`` / ``quantizer=`` kwargs or set the
  ``AUDIOTOKEN_*`` environment variables (configs.py); with nothing given, synthetic weights are used and a
  warning is logged.
* ``compile`` is accepted and ignored (there is no tracing compiler in the path; kernels are precompiled HIP).
* ``encode_batch_files`` shards files over ranks when ``torch.distributed`` is initialised (one process per GPU).
"""
from __future__ import annotations

import os
from pathlib import Path
from typing import Callable, List, Optional, Union

import numpy as np
import torch

from . import encode_files as EF
from . import runs
from .configs import (AcousticDecoderConfig, AcousticEncoderConfig, EncoderConfig, HubertEncoderConfig, Tokenizers, Wav2VecBertConfig,
                      num_codebooks_to_bandwidth)
from .harness import sanitize_path
from .logger import get_logger

logger = get_logger(__name__, log_file=None, level="WARNING")


class AudioToken:
    def __init__(self, tokenizer: Tokenizers, device: str = "cpu", compile: bool = False, **kwargs):
        """Reference ``AudioToken.__init__`` (core.py:28-71). Supported kwargs: ``num_codebooks`` in {2,4,8,16}
        (default 16 — the reference's actual default, core.py:67), ``weights``, ``quantizer``."""
        self.tokenizer_name = Tokenizers(tokenizer)  # ValueError on unknown names, like the reference's StrEnum
        self.encoder: Optional[torch.nn.Module] = None
        self.decoder: Optional[torch.nn.Module] = None
        self.model_config: EncoderConfig
        self.transform_func: Optional[Callable] = None
        self.compile = compile
        self.kwargs = kwargs
        self.device = device
        self.skipped_files: List[tuple] = []   # (path, reason) of the inputs the last encode_batch_files could not decode
        self.rank_probe: Optional[dict] = None    # checksums of the multi-rank start-up probe (load_encoder under torch.distributed), else None
        self.num_codebooks = kwargs.get("num_codebooks", 16)
        assert self.num_codebooks in [2, 4, 8, 16], "num_codebooks must be one of [2, 4, 8, 16]"
        self.load_config()

    def load_config(self):
        """core.py:73-90."""
        if self.tokenizer_name == Tokenizers.acoustic:
            self.model_config = AcousticEncoderConfig(bandwidth=num_codebooks_to_bandwidth(self.num_codebooks))
        elif self.tokenizer_name == Tokenizers.semantic_s:
            self.model_config = HubertEncoderConfig()
        elif self.tokenizer_name == Tokenizers.semantic_m:
            self.model_config = Wav2VecBertConfig()
        else:
            raise ValueError(f"Tokenizer {self.tokenizer_name} not supported")
        if self.kwargs.get("weights") is not None and not isinstance(self.kwargs["weights"], dict):
            self.model_config.weights = self.kwargs["weights"]
        if self.kwargs.get("quantizer") is not None and hasattr(self.model_config, "quantizer_path"):
            self.model_config.quantizer_path = self.kwargs["quantizer"]
        self.model_sample_rate = self.model_config.model_sample_rate

    def _weights_kw(self):
        w = self.kwargs.get("weights")
        return w if isinstance(w, dict) else None

    def load_encoder(self):
        """core.py:92-118 (lazy construction on first use). The reference is single-device; here, when ``torch.distributed`` is initialised with more than one
        rank, the model is built ONCE: rank 0 reads the checkpoint (the ``weights=`` path / dict, the ``AUDIOTOKEN_*`` variables, or the synthetic default),
        the other ranks receive it over RCCL — EnCodec as one flat tensor, the semantic tokenizers as rank 0's FINALIZED model (one packed device blob:
        no N-fold checkpoint read, fold, upload or split; distributed.encoder_on_all_ranks) — and every rank then encodes the same 2-clip probe: a rank whose
        tokens differ from rank 0's raises on ALL ranks before the first batch (``self.rank_probe`` keeps the checksums). ``broadcast_weights=False`` keeps
        per-rank loading (every rank must then be given the same checkpoint; the probe still runs unless ``rank_probe=False``). Collective: every rank of the
        group must construct its ``AudioToken`` and reach its first ``encode*`` call."""
        if self.encoder is not None:
            return
        from . import distributed as D
        dist = D.active()
        dev = torch.device(self.device)
        shared = dist is not None and self.kwargs.get("broadcast_weights", True)
        wkw = self._weights_kw()
        if self.tokenizer_name == Tokenizers.acoustic:
            from .encoder import AcousticEncoder
            if shared:
                from .encoder import encodec_weights_from
                wkw = D.weights_on_all_ranks(lambda: encodec_weights_from(wkw if wkw is not None else self.model_config.weights, with_decoder=False),
                                             dev, dist, "acoustic encoder")
            self.encoder = AcousticEncoder(device=self.device, config=self.model_config, weights=wkw)
        elif self.tokenizer_name == Tokenizers.semantic_s:
            from .hubert import HubertEncoder, hubert_processor
            local = lambda: HubertEncoder(config=self.model_config, device=self.device, weights=wkw)
            self.encoder = (D.encoder_on_all_ranks(local, lambda p: HubertEncoder(config=self.model_config, device=self.device, packed=p), dev, dist, "semantic_s encoder")
                            if shared else local())
            self.transform_func = hubert_processor
        elif self.tokenizer_name == Tokenizers.semantic_m:
            from .encoder import Wav2VecBertEncoder
            local = lambda: Wav2VecBertEncoder(config=self.model_config, device=self.device, quantize=True, weights=wkw)
            self.encoder = (D.encoder_on_all_ranks(local, lambda p: Wav2VecBertEncoder(config=self.model_config, device=self.device, quantize=True, packed=p),
                                                   dev, dist, "semantic_m encoder") if shared else local())
        else:
            raise ValueError(f"Tokenizer {self.tokenizer_name} not supported")
        self.encoder.eval()
        self.rank_probe = None
        if dist is not None and self.kwargs.get("rank_probe", True):
            x = D.probe_batch(self.model_config.model_sample_rate, self.device, self.transform_func)
            self.rank_probe = D.ranks_agree_on_probe(lambda w: self.encoder(w, torch.ones_like(w)), x, dev, dist, str(self.tokenizer_name))

    def stream(self, batch: int = 1, sample_rate: Optional[int] = None):
        """A streaming acoustic encoder (``AcousticStream``: ``push`` / ``flush`` / ``reset``) for audio that arrives in pieces; the concatenated
        tokens are those of one-shot ``encode``. The semantic tokenizers are not causal and have no streaming form.
        ``sample_rate``: ``push`` takes raw samples at that rate (float32 or int16, torch or numpy); they are resampled on the device as ONE signal
        (DESIGN.md §16), so the tokens are those of the whole signal resampled once, whatever the pushes. None: float samples at the model's rate."""
        if self.tokenizer_name != Tokenizers.acoustic:
            raise ValueError(f"streaming is available for Tokenizers.acoustic only (EnCodec is causal); {self.tokenizer_name} has no streaming form")
        self.load_encoder()
        return self.encoder.new_stream(batch) if sample_rate is None else self.encoder.new_stream(batch, sample_rate=sample_rate)

    def stream_pool(self, slots: int = 1):
        """Up to ``slots`` acoustic streams that start and finish on their own (``AcousticStreamPool``: ``open`` / ``push({id: samples})`` / ``flush`` /
        ``close``), batched per call by phase and length. Acoustic only, as ``stream()``. ``open(sample_rate=r)`` opens a stream that is pushed raw
        samples at ``r`` Hz; streams of different rates in one call share one resample launch."""
        if self.tokenizer_name != Tokenizers.acoustic:
            raise ValueError(f"streaming is available for Tokenizers.acoustic only (EnCodec is causal); {self.tokenizer_name} has no streaming form")
        self.load_encoder()
        return self.encoder.new_stream_pool(slots)

    def encode(self, audio: Union[torch.Tensor, np.ndarray, os.PathLike, bytes, Path], chunk_size: Optional[int] = None,
               stream: bool = False, resample: str = "chunk") -> torch.Tensor:
        """core.py:120-185. ``(1, num_samples)`` array/tensor or a path -> tokens ``(1, K, T)`` on the CPU
        (``(K, sum T)`` when a path is encoded with ``chunk_size`` — the reference drops the batch dim there).
        ``stream=True`` with a path and ``chunk_size`` (acoustic only) pushes the chunks through ONE stream instead of encoding each as a clip of
        its own: the result is the whole file's ``(1, K, ceil(N/320))`` in the memory of one chunk. A file that is not at the model's rate is resampled
        chunk by chunk on the host with ``resample="chunk"`` (the reference's seams); ``resample="file"`` (needs ``stream=True``) keeps its PCM on the
        device and resamples it as ONE signal: the tokens of the whole file resampled once, whatever ``chunk_size``."""
        self._check_resample(resample, stream)
        if stream:
            if not (isinstance(audio, (os.PathLike, Path)) and chunk_size is not None):
                raise ValueError("stream=True needs a path and a chunk_size (arrays and whole files are encoded one-shot)")
            if resample == "file":
                return self._encode_resident(audio, chunk_size)
            from .audio_io import process_audio_chunks
            st = self.stream(1)
            parts = [st.push(chunk) for chunk, _ in process_audio_chunks(audio, self.model_config.model_sample_rate, chunk_size)]
            parts.append(st.flush())
            return torch.cat([p.cpu() for p in parts], dim=-1)
        self.load_encoder()
        if isinstance(audio, np.ndarray):
            assert audio.ndim == 2, "Audio must be 2D array"
            assert audio.shape[0] == 1, "Audio must mono"
            return self._encode_single(torch.from_numpy(audio))
        elif isinstance(audio, torch.Tensor):
            assert audio.ndim == 2, "Audio must be 2D array"
            assert audio.shape[0] == 1, "Audio must mono"
            return self._encode_single(audio)
        elif isinstance(audio, os.PathLike) or isinstance(audio, Path):
            from .audio_io import process_audio_chunks, read_audio
            if chunk_size is None:
                logger.warning("Chunking not provided. Encoding the complete audio file at once. May run out of memory for larger audio files.")
                return self._encode_single(read_audio(audio, self.model_config.model_sample_rate))
            processed = [self._encode_single(chunk)[0]
                         for chunk, _ in process_audio_chunks(audio, self.model_config.model_sample_rate, chunk_size)]
            return torch.cat(processed, dim=-1)
        elif isinstance(audio, bytes):
            raise NotImplementedError("Encoding bytes not supported yet")
        else:
            raise ValueError(f"Unsupported input type {type(audio)}. Should be one of: {np.ndarray, os.PathLike, bytes, Path}")

    @staticmethod
    def _check_resample(resample, stream: bool) -> None:
        if resample not in ("chunk", "file"):
            raise ValueError(f"resample must be 'chunk' (every chunk resampled on its own) or 'file' (the file resampled as one signal), not {resample!r}")
        if resample == "file" and not stream:
            raise ValueError("resample='file' needs stream=True: only a streamed encode carries a file across its chunks")

    def _encode_resident(self, path, chunk_size) -> torch.Tensor:
        """``encode(path, chunk_size, stream=True, resample="file")``: the file's PCM on the device once, one resample launch and one push per tick."""
        from .audio_io import AudioDecodeError
        from .resample_stream import ResidentFiles
        st = self.stream(1)
        why = []
        src = ResidentFiles(self.device, self.model_config.model_sample_rate, chunk_size, 0, lambda name, reason: why.append(reason),
                            max_file_bytes=self.kwargs.get("max_file_bytes", 4 << 30))
        files = list(src.open_all([str(path)]))
        if len(files) != 1:
            raise AudioDecodeError(why[0] if why else f"{path}: one audio file expected, found {len(files)}")
        parts = [st.push(src.chunks([(files[0], c)])[0][None]) for c in range(files[0].ticks)]
        parts.append(st.flush())
        src.finish()
        return torch.cat([p.cpu() for p in parts], dim=-1)

    def _encode_single(self, audio: torch.Tensor) -> torch.Tensor:
        """core.py:187-196."""
        if self.transform_func:
            audio = self.transform_func(audio)
        input_batch = audio.to(self.device)
        attention_mask = torch.ones_like(input_batch, device=self.device)
        toks = self.encoder(input_batch, attention_mask)
        out = toks.cpu()                      # the reference's synchronisation point
        if hasattr(self.encoder, "verified"):  # device status of that call (LSTM hand-off / fp16 range): repeat on the safe path if set
            checked = self.encoder.verified(toks, input_batch, attention_mask)
            if checked is not toks:
                out = checked.cpu()
        return out

    def _chunk_stream(self, files, chunk_size: int, num_workers: int = 0, worker_processes: bool = False):
        """The host data flow of ``encode_batch_files``: file -> ``chunk_size``-second chunks -> segments, in order (encode_files.ChunkStream)."""
        skipped = runs.RunLog(self, "encode_batch_files").skipped
        return EF.ChunkStream(self, skipped, chunk_size, num_workers, worker_processes).segments(files)

    def encode_batch_files(self, batch_size: int, outdir: os.PathLike, chunk_size: int = 30, num_workers: int = 12,
                           audio_files: Optional[List[os.PathLike]] = None, audio_dir: Optional[Union[os.PathLike, Path]] = None,
                           stream: bool = False, resample: str = "chunk", **dataloader_kwargs) -> None:
        """core.py:198-289. Files -> ``chunk_size``-second segments -> batches -> encoder -> per-row trimmed
        ``<stem>.npy`` (append semantics as in the reference). ``num_workers`` files are decoded ahead of the device, in order (the reference's
        DataLoader workers; 0 = inline). On a HIP device, for the tokenizers without a host-side transform (acoustic, semantic_m), the samples never become
        float32 on the host: the DEVICE FEEDER (feeder.py) uploads the decoded PCM and converts / resamples / segments / pads in one kernel per batch
        (``device_feeder=False`` keeps the reference's host data flow). Host path: a thread pool by default — the heavy work (file read, FLAC decode, the
        resampling conv1d) releases the GIL — or spawned worker PROCESSES with ``worker_processes=True`` (the reference's arrangement; archives are always
        streamed by a thread). Under ``torch.distributed`` every rank takes whole files, balanced by size (distributed.shard_by_size): all chunks of a file stay
        on one rank, preserving the append order (``shard_across_ranks=False``: this rank takes every file it was given — for callers that have already
        split the work, e.g. one directory per rank).
        ``stream=True`` (acoustic only): every file is ONE clip — its token file is the ``[K, ceil(N / 320)]`` that
        ``encode(path, chunk_size, stream=True)`` returns, not the concatenation of per-chunk clips. Up to ``batch_size`` files are live at once, one slot of
        a stream pool each; per tick every live file pushes its next ``chunk_size`` seconds and the new frames are appended to its ``.npy``. A file that is
        not at the model's rate is still resampled chunk by chunk (``process_audio_chunks``), so its resampling seams remain: for such a file "the whole
        file" means the concatenated resampled chunks. Plain audio files only: an archive is recorded in ``skipped_files``.
        ``resample="file"`` (needs ``stream=True``) removes those seams: the device feeder's decoders read the files ahead in their storage
        format, a live file's PCM stays on the device from its first tick to its flush, and every tick ONE launch resamples the next chunk of every live
        file at file-global positions — the token file is that of the whole file resampled once. Archive members stream like files. A file whose PCM
        exceeds ``max_file_bytes`` (keyword, default 4 GiB) or that is not mono is recorded in ``skipped_files``."""
        self._check_resample(resample, stream)
        if stream and self.tokenizer_name != Tokenizers.acoustic:
            raise ValueError(f"streaming is available for Tokenizers.acoustic only (EnCodec is causal); {self.tokenizer_name} has no streaming form")
        self.load_encoder()
        self.skipped_files = []
        assert audio_files or audio_dir, "Either audio_files or audio_dir must be provided"
        assert not (audio_files and audio_dir), "Provide either audio_files or audio_dir, not both"
        outdir = sanitize_path(outdir)
        files = self._input_files(audio_files, audio_dir)
        files = runs.shard_if_distributed(self, files, dataloader_kwargs.get("shard_across_ranks", True))
        EF.encode_files(self, files, batch_size, outdir, chunk_size, num_workers, audio_files, audio_dir, stream, resample, dataloader_kwargs)

    @staticmethod
    def _input_files(audio_files, audio_dir, exts=None) -> List[str]:
        """The inputs of encode_batch_files / fit_quantizer / decode_batch_files (runs.input_files)."""
        return runs.input_files(audio_files, audio_dir, exts)

    def _shard_files(self, files: List[str]) -> List[str]:
        """This rank's share of the file list under torch.distributed (collective: every rank calls it with the same list; runs.shard_files)."""
        return runs.shard_files(self, files)

    # code-book sizes the tokenizers' finalize() accepts (csrc/w2vbert.hip, csrc/hubert.hip): (clusters, width, LayerNorm kernel of the quantiser step)
    _FIT_SHAPES = {Tokenizers.semantic_m: (2048, 1024, 1), Tokenizers.semantic_s: (1000, 768, 0)}

    def fit_quantizer(self, path: os.PathLike, audio_dir: Optional[Union[os.PathLike, Path]] = None, audio_files: Optional[List[os.PathLike]] = None,
                      chunk_size: int = 30, batch_size: int = 64, num_workers: int = 0, max_frames: int = 4_000_000, keep_fraction: float = 1.0,
                      num_clusters: Optional[int] = None, max_iter: int = 150, tol: float = 1e-4, seed: int = 0, n_init: int = 1, init="k-means++",
                      **dataloader_kwargs):
        """Fit the semantic tokenizer's code book on a corpus (the reference's scripts/clustering/cluster_tokens.py) and write it to ``path`` in the format
        the tokenizer loads (semantic_m: the VectorQuantize state dict, semantic_s: the joblib k-means). Frames: the encoder's hidden state with
        ``quantize=False`` through the checked encode path (a batch that overflowed the fp16 range is re-encoded by ``verified`` before it adds frames),
        segments cut as ``encode_batch_files`` cuts them, only each segment's valid frames (``length_tokens``), normalised by the quantiser step's own
        LayerNorm kernel, in file / segment / frame order. ``keep_fraction`` keeps a frame by a counter-based draw keyed on (file, segment, frame);
        ``max_frames`` caps the sample. Local to this process: no collectives, also under torch.distributed. Returns the fitted ``KMeans``."""
        from . import _cabi
        from .kmeans import KMeans, save_kmeans, save_vq
        if self.tokenizer_name not in self._FIT_SHAPES:
            raise ValueError(f"fit_quantizer: {self.tokenizer_name} has no semantic code book to fit (semantic_m or semantic_s)")
        k, d, split_ln = self._FIT_SHAPES[self.tokenizer_name]
        if num_clusters is not None and int(num_clusters) != k:
            raise ValueError(f"fit_quantizer: {self.tokenizer_name} quantises against exactly {k} codes, not {num_clusters}")
        if not 0.0 < float(keep_fraction) <= 1.0:
            raise ValueError(f"fit_quantizer: keep_fraction must be in (0, 1], got {keep_fraction}")
        if int(max_frames) < k:
            raise ValueError(f"fit_quantizer: max_frames = {max_frames} < {k} codes")
        assert audio_files or audio_dir, "Either audio_files or audio_dir must be provided"
        assert not (audio_files and audio_dir), "Provide either audio_files or audio_dir, not both"
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise ValueError("fit_quantizer needs a HIP device")
        lib = _cabi.load()
        max_frames = int(max_frames)
        need = max_frames * d * 4 + int(lib.at_kmeans_device_bytes(max_frames, d, k))
        free = torch.cuda.mem_get_info(dev)[0]
        if need > free:
            raise ValueError(f"fit_quantizer: max_frames = {max_frames} needs {need / 2**30:.2f} GiB of device memory "
                             f"({max_frames * d * 4 / 2**30:.2f} GiB of frames + {(need - max_frames * d * 4) / 2**30:.2f} GiB of k-means state); "
                             f"{free / 2**30:.2f} GiB are free")
        # the encoder without a code book (hidden state out); the same checkpoint and layer as the tokenizer
        wkw = self._weights_kw()
        if self.tokenizer_name == Tokenizers.semantic_m:
            from .encoder import Wav2VecBertEncoder
            enc = Wav2VecBertEncoder(config=self.model_config, device=self.device, quantize=False, weights=wkw)
        else:
            from .hubert import HubertEncoder
            enc = HubertEncoder(config=self.model_config, device=self.device, quantize=False, weights=wkw)
        enc.eval()
        files = self._input_files(audio_files, audio_dir)
        self.skipped_files = []
        log = runs.RunLog(self, "fit_quantizer")
        fb0 = getattr(enc, "fallback_batches", 0)
        X, sample = EF.collect_frames(self, log, enc, files, chunk_size, batch_size, num_workers, max_frames, d, split_ln, keep_fraction, seed)
        if sample["truncated"]:
            logger.warning(f"fit_quantizer: the sample reached max_frames = {max_frames}; later frames were not used")
        if len(X) < k:
            raise ValueError(f"fit_quantizer: {len(X)} frames collected, fewer than the {k} codes to fit")
        km = KMeans(k, init=init, n_init=n_init, max_iter=max_iter, tol=tol, seed=seed, device=self.device)
        km.fit(X)
        km.fit_summary_ = {**sample, "fallback_batches": getattr(enc, "fallback_batches", 0) - fb0, "skipped_files": len(self.skipped_files)}
        if self.tokenizer_name == Tokenizers.semantic_m:
            save_vq(path, km.cluster_centers_)
        else:
            save_kmeans(path, km)
        return km

    def to_acoustic(self, tokens, max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100, seed: int = 0, uniforms=None,
                    constrain: bool = False, return_logits: bool = False, long_form: bool = False, window: Optional[int] = None, hop: Optional[int] = None,
                    slots: Optional[int] = None, tick_tokens: Optional[int] = None, voice=None, top_p: Optional[float] = None,
                    min_p: Optional[float] = None):
        """Semantic ids -> the two coarse EnCodec code books: stage 1 of the reference's semantic decoder (its GPT, ``decoder.py:210-239``) on the
        KV-cached HIP decoder (semantic_decoder.py). Semantic tokenizers only. ``tokens``: a tensor / array / path of semantic ids (any
        shape, flattened), or a list of up to 64 of them, generated as one batch. Returns an ``AcousticGeneration``: ``codes`` (a list of int64
        ``[2, T_b]`` that ``AudioToken(Tokenizers.acoustic, num_codebooks=2).decode`` takes; None where the ids do not deserialise), ``ids``,
        ``finish`` ("stop" | "max_new_tokens" | "block_size") and, with ``return_logits``, the per-step logits.
        The draws are ``uniforms`` (float32 ``[B, max_new_tokens]``) or, from ``seed``, ``np.random.Generator(np.random.Philox(seed)).random(...)``: not
        ``torch.multinomial``'s stream, but the same distribution. ``constrain=True`` lets step s produce only ids of code book ``s % 2`` (and STOP on even
        s), so that every result is a valid ``[2, T]``; the default samples the reference's unconstrained distribution. Weights: the constructor's
        ``decoder_weights=`` (a checkpoint path or a ``{name: array}`` dict), else the seeded synthetic model.
        Without ``long_form`` a source is cut to its first ``max_source_tokens`` ids (5 s), as the reference cuts it. ``long_form=True`` walks the whole
        source (up to 65536 ids) in windows of ``window`` ids every ``hop`` ids, carrying the acoustic ids of the overlap: always
        constrained, ``uniforms`` indexed by the position in the row's result, ``windows`` of the result the schedule that ran. With ``slots=`` (1 to 64) the
        long form takes 1 to 4096 sources and runs them through that many cache rows, each source starting when a row is free and finishing on its own
        (DESIGN.md §20); ``tick_tokens`` bounds the tokens of one model pass. A source's result does not depend on its neighbours.
        ``voice=`` (``long_form=True`` only): a ``VoicePrompt`` that every source continues, or a list with one (or None) per source. The
        prompt's ids stand in front of the source's and its coarse codes are the first window's carry; the result covers the generated ids only.
        ``top_p`` / ``min_p``: after the top-k, keep the ids whose mass strictly above them is below ``top_p`` of the top-k set's, and
        the ids whose probability is at least ``min_p`` times the largest; None (or 1 / 0) is off and draws exactly what the call drew without them."""
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"to_acoustic maps semantic ids to acoustic code books; {self.tokenizer_name} has no semantic ids")
        if not long_form and (window is not None or hop is not None):
            raise ValueError("to_acoustic: window= and hop= belong to long_form=True")
        if not long_form and (slots is not None or tick_tokens is not None):
            raise ValueError("to_acoustic: slots= and tick_tokens= belong to long_form=True")
        if not long_form and voice is not None:
            raise ValueError("to_acoustic: voice= belongs to long_form=True (the prompt is the first window's carry, which only the long form has)")
        self._gpt()
        if long_form:
            return self.semantic_decoder.to_acoustic_long(tokens, window=window, hop=hop, max_new_tokens=max_new_tokens, temperature=temperature, top_k=top_k,
                                                          seed=seed, uniforms=uniforms, return_logits=return_logits, slots=slots, tick_tokens=tick_tokens,
                                                          voice=voice, top_p=top_p, min_p=min_p)
        return self.semantic_decoder.to_acoustic(tokens, max_new_tokens=max_new_tokens, temperature=temperature, top_k=top_k, seed=seed, uniforms=uniforms,
                                                 constrain=constrain, return_logits=return_logits, top_p=top_p, min_p=min_p)

    def score_acoustic(self, tokens, codes, temperature: float = 1.0, constrain: bool = False, include_stop: bool = True, long_form: bool = False,
                       window: Optional[int] = None, hop: Optional[int] = None, return_logits: bool = False):
        """How likely given coarse codes are under the semantic decoder's GPT, teacher-forced: the evaluation half of the reference's model
        (``GPT.forward(idx, targets)``, ``gpt2_model.py:161-164``) on the HIP decoder (semantic_decoder.py). Nothing is drawn. Semantic
        tokenizers only. ``tokens`` as ``to_acoustic`` takes them: one source, or a list of up to 4096. ``codes``: integer ``[2, T]`` per source (of
        ``[K >= 2, T]`` rows 0 and 1), what ``AudioToken(Tokenizers.acoustic).encode`` and ``AcousticGeneration.codes`` give. A source's sequence is what
        generation would have written: ids + SEMANTIC_OFFSET, INFER, the codes interleaved (the inverse of ``coarse_codes``), then STOP with
        ``include_stop``; every acoustic position is scored. Returns an ``AcousticScore``: per source ``logprob`` and ``rank`` at stream positions (STOP
        last), ``nll`` (the mean of ``-logprob``, what the reference's cross-entropy gives the source alone) and, with ``return_logits``, the logits.
        The default scores the model's own distribution over all ids at ``temperature`` 1, the reference's cross-entropy. ``constrain=True`` scores under
        the allow sets ``to_acoustic(constrain=True)`` draws under, and with its ``temperature`` that is the distribution generation draws from before
        top-k; ``rank < top_k`` says whether top-k would have kept the id. A source longer than ``max_source_tokens`` is refused without ``long_form``:
        generation would cut it, and a cut here would score the wrong pairing. ``long_form=True`` walks ``acoustic_windows`` with ``window`` / ``hop`` as
        ``to_acoustic(long_form=True)`` does: window k sees its source ids and the carry out of the GIVEN codes and scores its own new ids, the final
        window everything that is left; always constrained; ``windows`` of the result is the schedule with the counts scored. Voice prompts, the fine
        stage and files are not scored."""
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"score_acoustic scores acoustic code books against semantic ids; {self.tokenizer_name} has no semantic ids")
        if not long_form and (window is not None or hop is not None):
            raise ValueError("score_acoustic: window= and hop= belong to long_form=True")
        if not long_form:   # refused before a model is built, by the rule and the configuration the decoder itself will use
            from .semantic_decoder import refuse_long_source, source_ids
            cfg = self._decoder_config()
            for t in tokens if isinstance(tokens, (list, tuple)) else [tokens]:
                refuse_long_source(int(source_ids(t, cfg).numel()), cfg)
        return self._gpt().score_acoustic(tokens, codes, temperature=temperature, constrain=constrain, include_stop=include_stop, long_form=long_form,
                                          window=window, hop=hop, return_logits=return_logits)

    def to_fine(self, codes, temperature: Optional[float] = 0.5, seed: int = 0, uniforms=None, return_logits: bool = False, slots: Optional[int] = None,
                history=None):
        """The two coarse EnCodec code books -> all eight: stage 2 of the reference's semantic decoder (bark's ``generate_fine``) on the HIP fine
        transformer (fine_decoder.py). Acoustic codes in, acoustic codes out, so every tokenizer has it. ``codes``: integer ``[2, T]``, or a
        list of up to 64 of them of their own lengths, run as one batch. Returns a ``FineGeneration``: ``codes`` (a list of int64 ``[8, T_b]`` that
        ``AudioToken(Tokenizers.acoustic, num_codebooks=8).decode`` takes) and, with ``return_logits``, the logits and ids of every window and pass.
        ``temperature=None`` takes the argmax; any number samples (1.0 too, where HF takes the argmax) with the draws ``uniforms`` (float32
        ``[B, n_max, 6, W]``) or, from ``seed``, ``np.random.Generator(np.random.Philox(seed)).random(...)`` of that shape. Weights: the constructor's
        ``fine_weights=`` (a checkpoint path or a ``{name: array}`` dict), else ``$AUDIOTOKEN_FINE_DECODER_WEIGHTS``, else the seeded synthetic model.
        With ``slots=`` (1 to 64) the call is the window queue and takes 1 to 4096 rows: each row starts when a work array is free and
        leaves after its last window, so a long row does not hold short ones back. ``uniforms`` is then a list of per-row float32 ``[n_b, 6, W]``; from
        ``seed`` row b draws ``np.random.Generator(np.random.Philox(key=[seed, b])).random((n_b, 6, W), float32)``, whatever the other rows are. A row's
        codes are those of the row alone with the same draws; the result also carries ``passes`` and ``placement``.
        ``history=`` makes the rows continue a clip (bark's ``history_prompt["fine_prompt"]``): integer ``[8, Th]`` EnCodec codes that
        every row continues, or a list with one such array (or None) per row. The last ``min(W / 2, Th)`` frames stand in front of the row's own and are
        read, never written; the result holds the row's own frames only, and a row's windows (which ``uniforms`` counts) are
        ``fine_decoder.fine_windows(T, W, history_cells(Th, W))``. Rows that name the SAME object share one entry of the device's table (one upload of its
        last ``W / 2`` frames for a whole corpus); equal arrays that are distinct objects are uploaded once each."""
        from .fine_decoder import MAX_SLOTS, _as_histories, _as_rows
        rows = _as_rows(codes)   # a malformed input is refused before any model is built
        _as_histories(history, len(rows), 0, check_only=True)   # so is a malformed history, by its shape and dtype alone: generate converts it, once
        if slots is not None:
            if not (isinstance(slots, (int, np.integer)) and 1 <= slots <= MAX_SLOTS):
                raise ValueError(f"to_fine: slots must be 1 to {MAX_SLOTS}, got {slots!r}")
            return self._fine().generate_queue(rows, slots=int(slots), temperature=temperature, seed=seed, uniforms=uniforms, return_logits=return_logits,
                                               history=history)
        return self._fine().generate(rows, temperature=temperature, seed=seed, uniforms=uniforms, return_logits=return_logits, history=history)

    def voice_prompt(self, path, max_ids: Optional[int] = None):
        """A ``VoicePrompt`` from an audio file: the file's semantic ids from this tokenizer's own encoder, its EnCodec codes from an
        acoustic tokenizer at 8 code books held the way ``to_audio`` holds its decoder, and of both the latest aligned stretch
        (``VoicePrompt.from_tokens``) of at most ``max_ids`` ids; default: window - hop of ``default_window``, the longest prompt the long form takes."""
        from .semantic_decoder import default_window
        from .voice import VoicePrompt
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"voice_prompt pairs semantic ids with acoustic codes; {self.tokenizer_name} has no semantic ids")
        gpt = self._gpt()
        if max_ids is None:
            S, H = default_window(gpt.config, gpt.block_size)
            max_ids = S - H
        path = Path(path)
        sem = self.encode(path)
        codes = self._fine_audio().encode(path)
        return VoicePrompt.from_tokens(torch.as_tensor(sem).cpu().reshape(-1), torch.as_tensor(codes).cpu().reshape(8, -1), int(max_ids),
                                       gpt.config.SEMANTIC_VOCAB_SIZE)

    def _decoder_config(self):
        """The semantic decoder's configuration of this tokenizer: the loaded decoder's own, else the one ``_gpt`` will build it with."""
        if getattr(self, "semantic_decoder", None) is not None:
            return self.semantic_decoder.config
        from .configs import HubertDecoderConfig, Wav2VecBertDecoderConfig
        return HubertDecoderConfig() if self.tokenizer_name == Tokenizers.semantic_s else Wav2VecBertDecoderConfig()

    def _gpt(self):
        if getattr(self, "semantic_decoder", None) is None:
            from .semantic_decoder import SemanticToAcoustic
            cfg = self._decoder_config()
            w = self.kwargs.get("decoder_weights")
            if w is None and cfg.weights is None:
                logger.warning("to_acoustic: no decoder_weights given; using the seeded synthetic GPT")
            self.semantic_decoder = SemanticToAcoustic(cfg, device=self.device, weights=w)
        return self.semantic_decoder

    def _fine_audio(self):
        """The acoustic tokenizer at 8 code books that decodes what ``to_fine`` produced."""
        if getattr(self, "fine_audio", None) is None:
            self.fine_audio = AudioToken(Tokenizers.acoustic, device=self.device, num_codebooks=8, weights=self.kwargs.get("acoustic_weights"))
        return self.fine_audio

    def _fine(self):
        if getattr(self, "fine_decoder", None) is None:
            from .configs import FineDecoderConfig
            from .fine_decoder import CoarseToFine
            cfg = FineDecoderConfig()
            w = self.kwargs.get("fine_weights")
            if w is None and cfg.weights is None:
                logger.warning("to_fine: no fine_weights given; using the seeded synthetic fine model")
            self.fine_decoder = CoarseToFine(cfg, device=self.device, weights=w)
        return self.fine_decoder

    def to_audio(self, tokens, max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100, fine_temperature: Optional[float] = 0.5,
                 seed: int = 0, uniforms=None, fine_uniforms=None, long_form: bool = False, window: Optional[int] = None, hop: Optional[int] = None,
                 slots: Optional[int] = None, tick_tokens: Optional[int] = None, voice=None, top_p: Optional[float] = None, min_p: Optional[float] = None):
        """Semantic ids -> audio, this project's form of the reference's semantic ``decode`` (``decoder.py:210-243``): ``to_acoustic(constrain=True)``, then
        ``to_fine``, then the acoustic decoder at 8 code books (bandwidth 6). Semantic tokenizers only. ``tokens`` as ``to_acoustic`` takes them. Returns
        ``(audio, coarse, fine)``: a list of one float32 ``(1, 320 * T_b)`` CPU tensor per source, the ``AcousticGeneration`` and the ``FineGeneration``.
        ``uniforms`` / ``fine_uniforms`` / ``seed`` are the two stages' draws. A source whose stage 1 produced no whole frame raises ``ValueError``.
        ``long_form=True`` (with ``window`` / ``hop``) makes stage 1 the long form of ``to_acoustic``, so that the audio covers the whole source and not its
        first 5 s; the two later stages take any length as they are. With ``slots=`` stage 1 is the generation queue and takes up to 4096 sources; ``to_fine``
        then runs in groups of at most 64 in source order (``fine_uniforms``: ``[B, n_max, 6, W]`` over all sources, each group taking its rows and the windows
        its longest member needs), and the returned ``FineGeneration`` holds every source's codes.
        ``voice=`` (``long_form=True`` only): a ``VoicePrompt`` with all 8 code books that every source continues, or a list with one (or
        None) per source: its ids and code books 0 and 1 prompt stage 1, all 8 are ``to_fine``'s ``history``. The audio and both generations cover the
        generated frames only. ``top_p`` / ``min_p`` are stage 1's (``to_acoustic``); the fine stage has no truncation."""
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"to_audio maps semantic ids to audio; {self.tokenizer_name} has no semantic ids (its own decode is the way back)")
        history = None
        if voice is not None:
            if not long_form:
                raise ValueError("to_audio: voice= belongs to long_form=True")
            from .voice import per_row
            n_src = len(tokens) if isinstance(tokens, (list, tuple)) else 1
            rows = per_row(voice, n_src, "to_audio: voice")
            if any(v is not None and v.codes.shape[0] != 8 for v in rows):
                raise ValueError("to_audio: a voice prompt needs all 8 code books (the fine stage continues them)")
            history = voice.codes if not isinstance(voice, (list, tuple)) else [None if v is None else v.codes for v in rows]
        coarse = self.to_acoustic(tokens, max_new_tokens=max_new_tokens, temperature=temperature, top_k=top_k, seed=seed, uniforms=uniforms, constrain=True,
                                  long_form=long_form, window=window, hop=hop, slots=slots, tick_tokens=tick_tokens, voice=voice, top_p=top_p, min_p=min_p)
        for b, c in enumerate(coarse.codes):
            if c is None or c.shape[1] < 1:
                raise ValueError(f"to_audio: source {b} produced no whole frame of coarse codes (finish: {coarse.finish[b]})")
        if len(coarse.codes) <= 64:
            fine = self.to_fine(coarse.codes, temperature=fine_temperature, seed=seed, uniforms=fine_uniforms, history=history)
        else:
            fine = self._to_fine_in_groups(coarse.codes, fine_temperature, seed, fine_uniforms, history=history)
        audio = [self._fine_audio().decode(c.unsqueeze(0)) for c in fine.codes]
        return audio, coarse, fine

    def audio_stream(self, window: Optional[int] = None, hop: Optional[int] = None, max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100,
                     fine_temperature: Optional[float] = 0.5, seed: int = 0, uniforms=None, fine_uniforms=None, top_p: Optional[float] = None,
                     min_p: Optional[float] = None, keep_codes: bool = False, voice=None):
        """``to_audio(long_form=True)`` as a stream (``SemanticAudioStream``): ``push(ids)`` semantic ids as they arrive, each call returns
        the audio that turned final (float32 ``(1, 320 * n)``, ``n`` possibly 0), ``flush()`` the rest. One source per stream (``reset()`` starts the next);
        several streams may be alive at once. The coarse ids and the fine codes are those of ``to_acoustic(long_form=True)`` and ``to_fine`` on the whole
        source with the same draws; the memory does not grow with the source. The first audio of a long source needs ``W`` coarse frames (the fine model is
        non-causal over its window): 2048 GPT ids, 683 source ids at the product sizes; then audio arrives every ``W / 2`` frames (6.8 s). A source
        shorter than ``W`` frames gets all its audio at ``flush()``. Semantic tokenizers only; ``voice=`` is not built for streams."""
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"to_audio maps semantic ids to audio; {self.tokenizer_name} has no semantic ids (its own decode is the way back)")
        if voice is not None:
            raise ValueError("audio_stream: voice= is not built for streams (the prompted schedule changes every window); use to_audio(long_form=True, voice=)")
        from .semantic_decoder import check_truncation
        from .semantic_stream import SemanticAudioStream
        check_truncation(top_p, min_p)
        acoustic = self._fine_audio()
        acoustic.load_decoder()
        return SemanticAudioStream(self._gpt(), self._fine(), acoustic.decoder, window=window, hop=hop, max_new_tokens=max_new_tokens, temperature=temperature,
                                   top_k=top_k, fine_temperature=fine_temperature, seed=seed, uniforms=uniforms, fine_uniforms=fine_uniforms, top_p=top_p,
                                   min_p=min_p, keep_codes=keep_codes)

    def audio_stream_pool(self, streams: int = 64, slots: int = 16, fine_slots: int = 4, window: Optional[int] = None, hop: Optional[int] = None,
                          max_new_tokens: int = 1024, temperature: float = 0.8, top_k: int = 100, top_p: Optional[float] = None, min_p: Optional[float] = None,
                          fine_temperature: Optional[float] = 0.5, tick_tokens: Optional[int] = None, keep_codes: bool = False, return_logits: bool = False,
                          voice=None):
        """Up to ``streams`` live ``audio_stream()``s on one device state (``SemanticAudioStreamPool``): ``a = pool.open(seed=0)``;
        ``pool.push({a: ids_a, b: ids_b}, flush=[c])`` returns ``{sid: float32 (1, 320 n)}`` on the CPU for every stream named; ``pool.flush([a])``;
        ``pool.close(a)``; ``pool.stream(a)`` is the stream's record. A stream opened with seed ``s`` has the windows and draws of ``audio_stream(seed=s)``.
        The streams share ``slots`` (1 to 64) GPT cache rows tick by tick, fine passes of up to ``fine_slots`` windows, and one decode stream pool. One call
        is checked whole before anything is launched. Semantic tokenizers only; ``voice=`` is not built for streams."""
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"to_audio maps semantic ids to audio; {self.tokenizer_name} has no semantic ids (its own decode is the way back)")
        if voice is not None:
            raise ValueError("audio_stream: voice= is not built for streams (the prompted schedule changes every window); use to_audio(long_form=True, voice=)")
        from .semantic_decoder import check_truncation
        from .semantic_pool import MAX_POOL_STREAMS, SemanticAudioStreamPool
        check_truncation(top_p, min_p)
        if not 1 <= int(streams) <= MAX_POOL_STREAMS:
            raise ValueError(f"audio_stream_pool: streams must be 1 to {MAX_POOL_STREAMS}, got {streams}")
        decode_pool = self._fine_audio().decode_stream_pool(slots=int(streams))
        return SemanticAudioStreamPool(self._gpt(), self._fine(), decode_pool, streams=streams, slots=slots, fine_slots=fine_slots, window=window, hop=hop,
                                       max_new_tokens=max_new_tokens, temperature=temperature, top_k=top_k, top_p=top_p, min_p=min_p,
                                       fine_temperature=fine_temperature, tick_tokens=tick_tokens, keep_codes=keep_codes, return_logits=return_logits)

    def to_audio_batch_files(self, batch_size: int, outdir: os.PathLike, token_files: Optional[List[os.PathLike]] = None,
                             token_dir: Optional[Union[os.PathLike, Path]] = None, chunk_size: Optional[int] = None, num_workers: int = 12,
                             audio_format: str = "wav", rescale: bool = False, stream: bool = False, seed: int = 0, temperature: float = 0.8,
                             top_k: int = 100, fine_temperature: Optional[float] = 0.5, max_new_tokens: int = 1024, window: Optional[int] = None,
                             hop: Optional[int] = None, slots: int = 64, fine_slots: int = 64, round_files: int = 1024,
                             codes_dir: Optional[os.PathLike] = None, voice=None, top_p: Optional[float] = None, min_p: Optional[float] = None,
                             **kwargs) -> None:
        """The way back from a semantic ``encode_batch_files``: ``.npy`` files of semantic ids -> audio files (semantic_files.py). Semantic
        tokenizers only (``decode_batch_files`` stays the acoustic tokenizer's, and keeps raising here). Inputs, output names, overwriting, the skipping of
        a second input that maps to one output name, sharding under ``torch.distributed``, ``audio_format`` ("wav" / "flac", checked before any model is
        built), ``rescale``, ``stream``, ``run_summary`` / ``run_timings`` and ``skipped_files`` are ``decode_batch_files``'. An input is int16 / int64
        ``[T]``, ``[1, T]`` or ``[1, 1, T]``; one that is unreadable, of another dtype or rank, empty, longer than 65536 ids, holds an id outside the
        semantic vocabulary, or whose stage 1 produced no whole frame is skipped with its reason and the run goes on.
        The valid sources are taken ``round_files`` (1 to 4096) at a time: ``to_acoustic(long_form=True, slots=slots, window=, hop=, ...)`` (the GPT's
        generation queue), then ``to_fine(slots=fine_slots)`` (the fine stage's window queue, rows handed over longest first), and each file's ``[8, T]``
        codes go through the decode run of ``decode_batch_files`` at 8 code books: ``chunk_size=None`` decodes a file as one clip, ``stream=True`` pushes
        it through the decode stream pool. A round is generated when the decode side needs it: one round's ids and one decode batch's audio are held.
        ``codes_dir=`` also writes each file's codes as ``<same relative stem>.npy`` (int16 ``[8, T]``), which ``decode_batch_files`` reads.
        A file's draws (``semantic_files.file_draws``) come from ``np.random.Generator(np.random.Philox(key=[seed, fnv1a64(stem)]))``, ``stem`` its output
        path relative to ``outdir`` without the extension, in posix form: first the stage 1 draws of the source's own stream capacity, then its
        ``[n, 6, W]`` fine draws, so they do not depend on the other files, the round size or the ranks. ``run_summary`` gains ``rounds``, ``gpt_ticks``,
        ``fine_passes`` and ``generated_frames``; ``run_timings`` gains ``gpt_s`` and ``fine_s`` (both inside ``stage_s``).
        ``voice=``: one ``VoicePrompt`` with all 8 code books that every file continues, as ``to_audio(long_form=True, voice=)`` does; a
        file's ids and the prompt's may have 65536 together, and a file's fine draws count the windows of a row after the prompt's history.
        ``top_p`` / ``min_p``: stage 1's truncation after the top-k, checked before any model is built; None: off."""
        from . import semantic_files as SF
        from . import writer as Wr
        from .semantic_decoder import check_truncation
        if audio_format not in Wr.AUDIO_FORMATS:
            raise ValueError(f"audio_format must be one of {Wr.AUDIO_FORMATS}, got {audio_format!r}")
        check_truncation(top_p, min_p)
        if self.tokenizer_name not in (Tokenizers.semantic_s, Tokenizers.semantic_m):
            raise ValueError(f"to_audio_batch_files maps files of semantic ids to audio files; {self.tokenizer_name} has no semantic ids "
                             "(decode_batch_files is its way back)")
        assert token_files or token_dir, "Either token_files or token_dir must be provided"
        assert not (token_files and token_dir), "Provide either token_files or token_dir, not both"
        for name, value, most in (("slots", slots, 64), ("fine_slots", fine_slots, 64), ("round_files", round_files, 4096)):
            if not (isinstance(value, (int, np.integer)) and 1 <= value <= most):
                raise ValueError(f"to_audio_batch_files: {name} must be 1 to {most}, got {value!r}")
        known = {"shard_across_ranks", "device_writer", "max_held_bytes"}
        decoder_kwargs = {k: v for k, v in kwargs.items() if k not in known}
        stages = SF.Stages(self, seed, temperature, top_k, fine_temperature, max_new_tokens, window, hop, slots, fine_slots, voice=voice, top_p=top_p, min_p=min_p)
        acoustic = self._fine_audio()
        acoustic.load_decoder(**decoder_kwargs)
        self.skipped_files = []
        outdir = sanitize_path(outdir)
        files = self._input_files(token_files, token_dir, exts=(".npy",))
        files = runs.shard_if_distributed(self, files, kwargs.get("shard_across_ranks", True))
        log = runs.RunLog(self, "to_audio_batch_files", "audio")
        inputs, taken = [], {}
        for f in files:
            out = Wr.output_path(f, outdir, None if token_files else str(token_dir), audio_format)
            if out in taken:
                log.skipped(f, f"duplicate output name: {out} is already written from {taken[out]}")
                continue
            taken[out] = f
            inputs.append((f, out))
        on_gpu = torch.device(self.device).type == "cuda"
        cfg = acoustic.model_config
        SF.to_audio_files(self, acoustic.decoder, inputs, outdir, stages, self._gpt().config.SEMANTIC_VOCAB_SIZE, int(round_files), codes_dir,
                          int(batch_size), chunk_size, int(num_workers), bool(rescale), bool(kwargs.get("device_writer", on_gpu)),
                          int(kwargs.get("max_held_bytes", Wr.DEFAULT_MAX_HELD_BYTES)), cfg.model_sample_rate, cfg.model_token_rate, audio_format,
                          bool(stream), log=log)

    def _to_fine_in_groups(self, codes, temperature, seed, uniforms, group: int = 64, history=None):
        """``to_fine`` over more than 64 rows: groups of at most ``group`` in order, one ``FineGeneration`` over all of them. A group's draws are its rows of
        ``uniforms`` cut to the windows its longest member has; from ``seed`` each group draws its own stream, seeded ``seed + its index``."""
        from .fine_decoder import fine_windows, history_cells
        W = self._fine().block_size
        hist = history if isinstance(history, (list, tuple)) else [history] * len(codes)
        out = None
        for g, at in enumerate(range(0, len(codes), group)):
            rows = codes[at:at + group]
            u = None
            if uniforms is not None:
                n_max = max(len(fine_windows(int(c.shape[1]), W, 0 if hh is None else history_cells(int(hh.shape[1]), W)))
                            for c, hh in zip(rows, hist[at:at + group]))
                u = np.ascontiguousarray(np.asarray(uniforms)[at:at + group, :n_max])
            part = self.to_fine(rows, temperature=temperature, seed=seed + g, uniforms=u,
                                history=history if not isinstance(history, (list, tuple)) else hist[at:at + group])
            if out is None:
                out = part
            else:
                out.codes.extend(part.codes)
        return out

    def load_decoder(self, **kwargs):
        """core.py:291-315. Built: the acoustic decoder. The semantic way back is built under its own names: ``to_acoustic`` (stage 1, semantic ids -> the
        two coarse code books, a GPT), ``to_fine`` (stage 2, code books 3 to 8) and ``to_audio`` (both, then the acoustic decoder). The semantic ``decode``
        and this loader keep raising ``NotImplementedError`` for the semantic tokenizers."""
        if self.decoder is None:
            if self.tokenizer_name == Tokenizers.acoustic:
                from .decoder import AcousticDecoder
                cfg = AcousticDecoderConfig(bandwidth=num_codebooks_to_bandwidth(self.num_codebooks))
                if self.kwargs.get("weights") is not None and not isinstance(self.kwargs["weights"], dict):
                    cfg.weights = self.kwargs["weights"]
                wkw = self._weights_kw()
                from . import distributed as D
                dist = D.active()
                if dist is not None and self.kwargs.get("broadcast_weights", True):   # as load_encoder: rank 0 reads the checkpoint, one RCCL broadcast
                    from .encoder import encodec_weights_from
                    wkw = D.weights_on_all_ranks(lambda: encodec_weights_from(wkw if wkw is not None else cfg.weights, with_decoder=True),
                                                 torch.device(self.device), dist, "acoustic decoder")
                self.decoder = AcousticDecoder(config=cfg, device=self.device, weights=wkw, **kwargs)
            elif self.tokenizer_name in (Tokenizers.semantic_s, Tokenizers.semantic_m):
                raise NotImplementedError("the semantic decode needs the bark fine model, which is not built; stage 1 (semantic ids -> two coarse code "
                                          "books) is AudioToken.to_acoustic")
            else:
                raise ValueError(f"Tokenizer {self.tokenizer_name} not supported")
            self.decoder.eval()

    def decode_stream(self, batch: int = 1, **kwargs):
        """A streaming acoustic decoder (``AcousticDecodeStream``: ``push`` / ``flush`` / ``reset``) for tokens that arrive frame by frame; the
        concatenated audio is that of one-shot ``decode``. The semantic tokenizers have no decoder here and no streaming form."""
        if self.tokenizer_name != Tokenizers.acoustic:
            raise ValueError(f"streaming decode is available for Tokenizers.acoustic only; {self.tokenizer_name} has no streaming form")
        self.load_decoder(**kwargs)
        return self.decoder.new_stream(batch)

    def decode_stream_pool(self, slots: int = 1, **kwargs):
        """Up to ``slots`` acoustic decode streams that start and finish on their own (``AcousticDecodeStreamPool``), batched per call by phase, K and
        number of frames. Acoustic only, as ``decode_stream()``."""
        if self.tokenizer_name != Tokenizers.acoustic:
            raise ValueError(f"streaming decode is available for Tokenizers.acoustic only; {self.tokenizer_name} has no streaming form")
        self.load_decoder(**kwargs)
        return self.decoder.new_stream_pool(slots)

    def decode(self, tokens: Union[torch.Tensor, np.ndarray, os.PathLike, Path], chunk_size: Optional[int] = None, stream: bool = False,
               **kwargs) -> torch.Tensor:
        """core.py:317-353: tokens ``(B, K, T)`` -> audio ``(1, B*320*T)`` on the CPU.
        ``stream=True`` with a ``chunk_size`` in seconds (acoustic only, ``B = 1``) pushes ``chunk_size * 75`` frames at a time through ONE stream:
        the whole clip's ``(1, 320*T)`` in the memory of one chunk."""
        if stream:
            if chunk_size is None:
                raise ValueError("stream=True needs a chunk_size (seconds of audio per push)")
            st = self.decode_stream(1, **kwargs)
            if isinstance(tokens, np.ndarray):
                tokens = torch.from_numpy(tokens)
            elif isinstance(tokens, (os.PathLike, Path)):
                tokens = torch.load(tokens, map_location="cpu")
            if not isinstance(tokens, torch.Tensor):
                raise ValueError(f"Unsupported input type {type(tokens)}. Should be one of: {np.ndarray, os.PathLike, Path}")
            if tokens.dim() == 2:   # (K, sum T), what encode(path, chunk_size) returns
                tokens = tokens.unsqueeze(0)
            assert tokens.dim() == 3 and tokens.shape[0] == 1, "streamed decode takes one clip: tokens (1, K, T) or (K, T)"
            step = max(1, int(round(chunk_size * self.model_config.model_token_rate)))
            parts = [st.push(tokens[:, :, t0:t0 + step]).cpu() for t0 in range(0, tokens.shape[-1], step)]
            parts.append(st.flush().cpu())
            return torch.cat(parts, dim=-1)
        self.load_decoder(**kwargs)
        if isinstance(tokens, np.ndarray):
            return self._decode_single(torch.from_numpy(tokens))
        elif isinstance(tokens, torch.Tensor):
            return self._decode_single(tokens)
        elif isinstance(tokens, os.PathLike) or isinstance(tokens, Path):
            tokens_mem = torch.load(tokens, map_location="cpu")
            return self._decode_single(tokens_mem)
        else:
            raise ValueError(f"Unsupported input type {type(tokens)}. Should be one of: {np.ndarray, os.PathLike, Path}")

    def decode_batch_files(self, batch_size: int, outdir: os.PathLike, chunk_size: Optional[int] = 30, num_workers: int = 12,
                           token_files: Optional[List[os.PathLike]] = None, token_dir: Optional[Union[os.PathLike, Path]] = None,
                           rescale: bool = False, audio_format: str = "wav", stream: bool = False, **kwargs) -> None:
        """The way back from ``encode_batch_files`` (reference scripts/detokenize_audio.py + utils.save_audio): ``.npy`` token files -> mono 16-bit PCM
        WAV files at 24 kHz, or with ``audio_format="flac"`` FLAC files of the same samples (``<stem>.flac``; compressed on the device, csrc/flac_encode.hip;
        anything but "wav" / "flac" raises ValueError before a decoder is loaded). Acoustic only. ``token_dir`` is walked once (sorted, dot-names skipped) and its relative tree is kept; ``token_files`` are
        written flat into ``outdir``; each input becomes ``<stem>.wav``. An existing output is OVERWRITTEN — unlike the encode side, which appends:
        appending audio to an earlier run's file has no use. A token file is int16 / int64 ``[K, T]`` or ``[1, K, T]``; one that is unreadable, has
        another rank, more code books than the model, no frames or a code outside [0, 1023] is skipped and recorded in ``self.skipped_files`` (as is the
        second of two inputs that map to one output name) and the run goes on. Segments mirror the encode side: every ``chunk_size * 75`` frames are
        decoded as a clip of their own (``chunk_size=None``: the file is one clip), batched by equal K, right-padded (with the "no code" value -1: zero embedding rows) and trimmed; every batch
        passes ``AcousticDecoder.verified``. Samples are clamped to +-0.99, or with ``rescale=True`` scaled by the FILE's min(0.99 / peak, 1) (the float rows
        of a file stay on the device until its last row is decoded; a file holding more than ``max_held_bytes`` is skipped), rounded half to even and
        narrowed to int16 on the device (writer.py; ``device_writer=False`` converts on the host by the same rule). ``num_workers`` files are read ahead, in
        order. Under ``torch.distributed`` whole files are sharded by size (``shard_across_ranks=False``: this rank takes every file it was given).
        ``self.run_summary`` / ``self.run_timings`` describe the run (``run_summary["audio_bytes"]``: the bytes of the files written).
        ``stream=True``: the way back from ``encode_batch_files(stream=True)`` — every token file is decoded as ONE clip (what
        ``decode(tokens, chunk_size, stream=True)`` returns for it), up to ``batch_size`` files at a time through a decode stream pool, ``chunk_size * 75``
        frames per file and tick; outputs, skipping rules and ``rescale`` are those above."""
        from . import writer as Wr
        if audio_format not in Wr.AUDIO_FORMATS:
            raise ValueError(f"audio_format must be one of {Wr.AUDIO_FORMATS}, got {audio_format!r}")
        if self.tokenizer_name != Tokenizers.acoustic:
            self.load_decoder()      # raises what `decode` raises for a tokenizer without a decoder
        assert token_files or token_dir, "Either token_files or token_dir must be provided"
        assert not (token_files and token_dir), "Provide either token_files or token_dir, not both"
        known = {"shard_across_ranks", "device_writer", "max_held_bytes"}
        decoder_kwargs = {k: v for k, v in kwargs.items() if k not in known}
        self.load_decoder(**decoder_kwargs)
        self.skipped_files = []
        outdir = sanitize_path(outdir)
        files = self._input_files(token_files, token_dir, exts=(".npy",))
        files = runs.shard_if_distributed(self, files, kwargs.get("shard_across_ranks", True))
        log = runs.RunLog(self, "decode_batch_files", "audio")
        inputs, taken = [], {}
        for f in files:
            out = Wr.output_path(f, outdir, None if token_files else str(token_dir), audio_format)
            if out in taken:
                log.skipped(f, f"duplicate output name: {out} is already written from {taken[out]}")
                continue
            taken[out] = f
            inputs.append((f, out))
        on_gpu = torch.device(self.device).type == "cuda"
        Wr.decode_files(self, inputs, int(batch_size), chunk_size, int(num_workers), bool(rescale), bool(kwargs.get("device_writer", on_gpu)),
                        int(kwargs.get("max_held_bytes", Wr.DEFAULT_MAX_HELD_BYTES)), self.model_config.model_sample_rate, self.model_config.model_token_rate,
                        audio_format, bool(stream), log=log)

    def _decode_single(self, tokens: torch.Tensor) -> torch.Tensor:
        """core.py:355-359."""
        input_batch = tokens.to(dtype=torch.long)
        toks = self.decoder(input_batch)
        out = toks.cpu()
        if hasattr(self.decoder, "verified"):
            checked = self.decoder.verified(toks, input_batch)
            if checked is not toks:
                out = checked.cpu()
        return out
