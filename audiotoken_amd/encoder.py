"""Encoder callables with the reference's protocol: ``encoder(input_batch, attention_mask) -> int16 [B, K, T]``
(reference audiotoken/encoder.py:29-186), backed by libaudiotoken_hip.so through the C ABI.

PyTorch is used for device tensors, the caching allocator (workspace) and the current stream only.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from typing import Dict, Optional, Union

import numpy as np
import torch

from . import _cabi, fallback
from . import weights as W
from ._handle import LibHandle, SemanticHandle
from .configs import AcousticEncoderConfig
from .logger import get_logger

logger = get_logger(__name__)


def encodec_bandwidth_to_nq(bandwidth: float) -> int:
    """``n_q = max(1, floor(bw*1000 / (log2(1024)*75)))`` — encodec ResidualVectorQuantizer
    (call site reference audiotoken/encoder.py:50-52)."""
    return int(max(1, math.floor(bandwidth * 1000 / (10 * 75))))


def fold_encodec_weights(w: Dict[str, np.ndarray]) -> Dict[str, np.ndarray]:
    """encodec checkpoint dict (weight_g / weight_v pairs) -> folded ``.weight`` tensors for the C ABI."""
    out: Dict[str, np.ndarray] = {}
    for k, v in w.items():
        if k.endswith(".weight_g"):
            base = k[: -len(".weight_g")]
            out[base + ".weight"] = W.fold_weight_norm(v, w[base + ".weight_v"])
        elif k.endswith(".weight_v"):
            continue
        elif k.endswith("._codebook.embed"):
            out[k] = np.ascontiguousarray(v, dtype=np.float32)
            e = torch.from_numpy(out[k])
            # |e|^2 exactly as the reference forms it: embed.t().pow(2).sum(0, keepdim=True)
            out[k[: -len("embed")] + "e2"] = e.t().pow(2).sum(0).numpy()
        elif k.startswith(("encoder.", "decoder.", "quantizer.")) and not k.endswith(("inited", "cluster_size", "embed_avg")):
            out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


def load_encodec_checkpoint(path: str) -> Dict[str, np.ndarray]:
    """Read an ``encodec_24khz-*.th`` state dict (torch.save format) into numpy arrays."""
    sd = torch.load(path, map_location="cpu", weights_only=True)
    return {k: v.float().numpy() for k, v in sd.items() if torch.is_tensor(v)}


def encodec_weights_from(weights, with_decoder: bool) -> Dict[str, np.ndarray]:
    """``weights`` as the constructors accept it — None (synthetic, seed 0, logged), a checkpoint path, or a name -> array dict — as the un-folded dict."""
    if weights is None:
        logger.warning("No EnCodec checkpoint given (weights=/AUDIOTOKEN_ENCODEC_WEIGHTS): using synthetic weights, seed 0")
        return W.synth_encodec_weights(seed=0, with_decoder=with_decoder)
    if isinstance(weights, (str, bytes, os.PathLike)):
        return load_encodec_checkpoint(weights)
    return weights


class _EncodecHandle(LibHandle):
    """Owns one ``at_encodec_t`` (device weights live inside the library)."""
    FAMILY = "encodec"

    def __init__(self, device: Union[str, torch.device], weights: Optional[Union[str, Dict[str, np.ndarray]]],
                 with_decoder: bool):
        def host_tensors():
            folded = fold_encodec_weights(encodec_weights_from(weights, with_decoder))
            return {k: v for k, v in folded.items() if with_decoder or not k.startswith("decoder.")}
        self._create(device, None, host_tensors, 1 if with_decoder else 0)

    def _finish_init(self) -> None:
        self.n_codebooks = self._fn("num_codebooks")(self.handle)


class _EncodecCallable(LibHandle, torch.nn.Module):
    """An encoder or a decoder over an ``_EncodecHandle`` of its own (``_h``)."""
    FAMILY = "encodec"
    lib = property(lambda self: self._h.lib)
    handle = property(lambda self: self._h.handle)

    def _open(self, device, weights, with_decoder: bool) -> None:
        self._h = _EncodecHandle(device, weights, with_decoder)
        self.device = self._h.device
        self._init_call_state()
        self.fallback_batches = 0    # batches `verified` repeated without the f16x2 kernels (fp16 range overflow)


class AcousticEncoder(_EncodecCallable):
    """Drop-in for reference ``AcousticEncoder`` (audiotoken/encoder.py:29-57)."""

    def __init__(self, config: AcousticEncoderConfig = None, device: str = "cuda:0",
                 weights: Optional[Union[str, Dict[str, np.ndarray]]] = None):
        super().__init__()
        config = config or AcousticEncoderConfig()
        self.config = config
        self._open(device, weights if weights is not None else config.weights, with_decoder=False)
        self.n_q = encodec_bandwidth_to_nq(config.bandwidth)
        if self.n_q > self._h.n_codebooks:
            raise ValueError(f"bandwidth {config.bandwidth} needs {self.n_q} codebooks, checkpoint has {self._h.n_codebooks}")
        self.nonfinite_batches = 0   # batches whose activations held a NaN / infinity at the quantiser (status bit 2)

    def _sized_workspace(self, B: int, N: int):
        """Workspace for a [B, N] encode. The conv stack runs in sub-batches of `subbatch` clips (default 256, which needs
        ~0.22 GB per clip-10-s); when the allocation does not fit, the sub-batch is halved (option "subbatch") and the
        request repeated — results do not depend on it (clips are independent), only the workspace size does."""
        lib = self._h.lib
        sub = getattr(self, "_subbatch", None)
        while True:
            nbytes = lib.at_encodec_workspace_bytes(self._h.handle, B, N)
            try:
                return nbytes, self._workspace(nbytes)
            except torch.OutOfMemoryError:
                sub = max(1, (sub or min(B, 256)) // 2)
                if sub < 1 or getattr(self, "_subbatch", None) == 1:
                    raise
                logger.warning(f"workspace of {nbytes / 2**30:.1f} GiB does not fit: conv-stack sub-batch -> {sub} clips")
                self.set_option("subbatch", sub)
                self._subbatch = sub
                torch.cuda.empty_cache()

    # the f16x2 kernel groups with a range check (SEANet convs, LSTM input projection, final conv, RVQ search): off for the repeat of an overflowing batch
    RANGE_OPTIONS = ("ih_f16x2", "chain_f16x2", "res_f16x2", "rvq_f16x2", "fin_f16x2")

    def verified(self, codes: torch.Tensor, input_batch: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Product-path guard, called where the caller synchronises anyway (tokens leaving the device). The status word of the call that
        produced `codes` decides (fallback.encodec_ladder):
        * bit 0, the persistent LSTM's hand-off timed out (another process on the GPU, a partitioned device: not all 256 workgroups
          resident): a property of the MACHINE — log it, switch to the per-step LSTM launches for the rest of the handle's life and repeat;
        * bit 1, an activation exceeded the fp16 range of the f16x2 kernels: a property of THIS BATCH — repeat it on the bf16x3 kernels (fp32
          exponent range), count it in ``fallback_batches`` and switch back: the next batch runs on f16x2 again (round 2 switched the
          handle for good, so one outlier batch halved the throughput of the rest of a run);
        * bit 2, a NaN / infinity reached the quantiser: counted in ``nonfinite_batches`` and logged, the ids are returned as they are."""
        return fallback.encodec_ladder(self, codes, lambda: self.forward(input_batch, attention_mask), input_batch.shape[0],
                                       self.RANGE_OPTIONS, "acoustic encode")

    @torch.no_grad()
    def forward(self, input_batch: torch.Tensor, attention_mask: Optional[torch.Tensor] = None,
                return_embeddings: bool = False):
        """``float32 [B, N]`` on the device (+ ignored mask) -> ``int16 [B, n_q, ceil(N/320)]`` on the device."""
        assert input_batch.dim() == 2, "input_batch must be [B, N]"
        x = input_batch.to(device=self.device, dtype=torch.float32).contiguous()
        B, N = x.shape
        T = -(-N // W.ENCODEC_HOP)
        lib = self._h.lib
        codes = torch.empty((B, self.n_q, T), dtype=torch.int16, device=self.device)
        emb = torch.empty((B, T, W.ENCODEC_DIM), dtype=torch.float32, device=self.device) if return_embeddings else None
        nbytes, ws = self._sized_workspace(B, N)
        t_out = C.c_int(0)
        with torch.cuda.device(self.device):
            stream = _cabi.current_stream_handle(self.device)
            rc = lib.at_encodec_encode_checked(self._h.handle, x.data_ptr(), 0, B, N, self.n_q, codes.data_ptr(), C.byref(t_out),
                                               _cabi.ptr(emb), ws.data_ptr(), nbytes, stream, self._status.data_ptr())
        _cabi.check(rc, "at_encodec_encode_checked")
        assert t_out.value == T
        logger.info(f'Codes shape: {codes.shape}')
        if return_embeddings:
            return codes, emb
        return codes

    def resampler(self):
        """The encoder's device resampler (resample_stream.DeviceResampler: its tables live on the device once per rate), made on first use."""
        if getattr(self, "_resampler", None) is None:
            from .resample_stream import DeviceResampler
            self._resampler = DeviceResampler(self.device, self.config.model_sample_rate)
        return self._resampler

    def new_stream(self, batch: int = 1, sample_rate: Optional[int] = None):
        """A stateful encoder for audio that arrives in pieces (audiotoken_amd/streaming.py): ``push`` / ``flush`` give the tokens one-shot
        ``forward`` gives for the concatenated audio, in memory bounded by the largest push. Streams of one encoder are independent.
        ``sample_rate``: the pushes are raw samples at that rate, resampled on the device as one signal."""
        from .streaming import AcousticStream
        return AcousticStream(self, batch, sample_rate=sample_rate)

    def new_stream_pool(self, slots: int = 1):
        """Up to ``slots`` streams that start and finish on their own (audiotoken_amd/streaming.py, AcousticStreamPool): each gives the tokens of its
        own audio, and the streams of one call that are in the same phase with the same length share one library push."""
        from .streaming import AcousticStreamPool
        return AcousticStreamPool(self, slots)


# ======================================================================================================
# semantic_m: Wav2Vec2-BERT + VQ
# ======================================================================================================
def frontend_tables() -> Dict[str, np.ndarray]:
    """Povey window and mel filter bank, built with the reference's formulas so the device uses the very same
    fp32 tables (reference audiotoken/processors.py:8-26,66-78; audiotoken/utils.py:286-328): triangles built in
    mel space over 256 bins of width 16000/512 from 20 Hz to 8 kHz (Kaldi mel), plus one zero row."""
    def hz2mel(f):
        return 1127.0 * torch.log(1.0 + (f / 700.0))

    filt = torch.linspace(hz2mel(torch.tensor(20.0)), hz2mel(torch.tensor(8000.0)), 80 + 2)
    fft_freqs = hz2mel((16000 / 512) * torch.arange(256))
    diff = torch.diff(filt)
    slopes = filt.unsqueeze(0) - fft_freqs.unsqueeze(1)
    fb = torch.maximum(torch.zeros(1), torch.minimum(-slopes[:, :-2] / diff[:-1], slopes[:, 2:] / diff[1:]))
    fb = torch.nn.functional.pad(fb, (0, 0, 0, 1))
    window = torch.pow(torch.hann_window(400, periodic=False), 0.85)
    return {"frontend.mel_filters": fb.numpy(), "frontend.window": window.numpy()}


W2VBERT_ARCH = {"hidden_size": 1024, "intermediate_size": 4096, "num_attention_heads": 16, "feature_projection_input_dim": 160,
                "position_embeddings_type": "relative_key", "left_max_position_embeddings": 64, "right_max_position_embeddings": 8,
                "conv_depthwise_kernel_size": 31, "hidden_act": "swish"}


def load_w2vbert_checkpoint(model_dir: str, quantizer_path: Optional[str]) -> Dict[str, np.ndarray]:
    """The reference's ``Wav2Vec2BertModel.from_pretrained(config.model_id)`` directory (``w2vbert2_l21/``: config.json +
    model.safetensors, possibly sharded, 21 conformer layers of which 19 are used) + the VQ ``.pkl`` state dict it ``torch.load``s
    (reference audiotoken/encoder.py:132,156-161; audiotoken/configs.py:114-134; audiotoken/utils.py:331-339) -> numpy dict."""
    W.check_hf_config(model_dir, W2VBERT_ARCH, "semantic_m checkpoint")
    w = W.read_hf_state_dict(model_dir, strip_prefixes=("wav2vec2_bert.",))
    if quantizer_path:
        sd = torch.load(quantizer_path, map_location="cpu", weights_only=True)
        if "_codebook.embed" not in sd:
            raise ValueError(f"{quantizer_path}: no '_codebook.embed' (expected a vector_quantize_pytorch VectorQuantize state dict)")
        w["vq._codebook.embed"] = sd["_codebook.embed"].float().numpy()
    return w


class Wav2VecBertEncoder(SemanticHandle, torch.nn.Module):
    """Drop-in for reference ``Wav2VecBertEncoder`` with ``quantize=True`` (audiotoken/encoder.py:111-186)."""
    FAMILY, LAYER_NOUN = "w2vbert", "conformer"

    def __init__(self, config=None, device: str = "cuda:0", quantize: bool = True,
                 weights: Optional[Union[str, Dict[str, np.ndarray]]] = None, packed=None):
        """``packed`` = ``(meta, blob)`` from another rank's ``export_packed()`` (``distributed.broadcast_packed``): the finalized model is rebuilt
        over that device blob — no checkpoint is read, nothing is uploaded or split here (``weights`` is ignored)."""
        super().__init__()
        from .configs import Wav2VecBertConfig
        config = config or Wav2VecBertConfig()
        self.config = config
        self.quantize = quantize
        self.output_layer = config.output_layer
        self._create(device, packed, lambda: self._host_tensors(weights if weights is not None else config.weights))

    def _host_tensors(self, weights) -> Dict[str, np.ndarray]:
        if weights is None:
            logger.warning("No Wav2Vec2-BERT checkpoint given (weights=/AUDIOTOKEN_W2VBERT_WEIGHTS): synthetic weights, seed 0")
            weights = W.synth_w2vbert_weights(n_layers=self.output_layer, seed=0, with_vq=True)
        elif isinstance(weights, (str, bytes)):
            weights = load_w2vbert_checkpoint(weights, self.config.quantizer_path)
        tensors = dict(frontend_tables())
        for k, v in weights.items():
            if k.startswith("encoder.layers."):
                if int(k.split(".")[2]) >= self.output_layer:   # layers past the consumed hidden state are dead compute
                    continue
            elif not k.startswith(("feature_projection.", "vq.")):
                continue
            tensors[k] = v
        if "vq._codebook.embed" in tensors:
            e = torch.from_numpy(np.ascontiguousarray(tensors["vq._codebook.embed"], dtype=np.float32)).reshape(-1, 1024)
            tensors["vq._codebook.e2"] = (e ** 2).sum(-1).numpy()   # y2 of vector_quantize_pytorch's cdist
        return tensors

    def verified(self, tokens: torch.Tensor, input_batch: torch.Tensor, mask: Optional[torch.Tensor] = None, **kw) -> torch.Tensor:
        """Product-path guard, called where the caller synchronises anyway: if the call that produced `tokens` reported an fp16 range
        overflow, log it, find the conformer layer that caused it, move THAT layer to the bf16x3 arithmetic (full fp32 exponent range) and repeat this
        batch (``fallback_batches``); every other layer stays on f16x2. The layer returns to f16x2 after the batch unless it is its PIN_AFTER-th overflowing
        batch (then it stays: ``pinned_layers``). The policy is fallback.semantic_ladder."""
        return fallback.semantic_ladder(self, tokens, lambda: self.forward(input_batch, mask, **kw), 0, self.LAYER_NOUN, "semantic_m encode")

    def site_scales(self) -> Dict[str, list]:
        """{site: [scale per conformer layer]} — the power of two each split site multiplies its activations by (16, or the provable scale of a
        LayerNorm-fed site whose gains are too large for 16: include/audiotoken_hip.h, at_w2vbert_site_scales)."""
        names = C.create_string_buffer(2048)
        ns = self.lib.at_w2vbert_range_sites(names, 2048)
        buf = (C.c_float * (64 * 16))()
        n = self.lib.at_w2vbert_site_scales(self.handle, buf, 64 * 16)
        if ns <= 0 or n < 0:
            raise _cabi.HipLibraryError(f"at_w2vbert_site_scales failed: {_cabi.last_error()}")
        keys = names.value.decode().split("\n")[:ns]
        return {k: [float(buf[l * ns + i]) for l in range(n // ns)] for i, k in enumerate(keys)}

    @torch.no_grad()
    def forward(self, input_batch: torch.Tensor, mask: Optional[torch.Tensor] = None, pad_to_multiple_of: int = 2,
                n_layers: Optional[int] = None, return_taps: bool = False):
        """``float32 [B, N]`` @16 kHz + ``float32 [B, N]`` mask -> ``int16 [B, 1, T']`` on the device.
        With ``quantize=False`` returns the selected hidden state ``[B, T', 1024]`` like the reference."""
        assert input_batch.dim() == 2, "Input tensor must have shape [batch, time]"
        x = input_batch.to(device=self.device, dtype=torch.float32).contiguous()
        m = None if mask is None else mask.to(device=self.device, dtype=torch.float32).contiguous()
        B, N = x.shape
        nl = self.output_layer if n_layers is None else n_layers
        T = self.lib.at_w2vbert_num_tokens(N, pad_to_multiple_of)
        want_tokens = self.quantize
        tokens = torch.empty((B, 1, T), dtype=torch.int16, device=self.device) if want_tokens else None
        feats = amask = hidden = None
        if return_taps or not want_tokens:
            hidden = torch.empty((B, T, 1024), dtype=torch.float32, device=self.device)
        if return_taps:
            feats = torch.empty((B, T, 160), dtype=torch.float32, device=self.device)
            amask = torch.empty((B, T), dtype=torch.float32, device=self.device)
        nbytes = self.lib.at_w2vbert_workspace_bytes(self.handle, B, N, pad_to_multiple_of)
        ws = self._workspace(nbytes)
        t_out = C.c_int(0)
        with torch.cuda.device(self.device):
            rc = self.lib.at_w2vbert_encode_checked(self.handle, x.data_ptr(), _cabi.ptr(m), B, N, pad_to_multiple_of, nl,
                                                    _cabi.ptr(tokens), C.byref(t_out), _cabi.ptr(feats), _cabi.ptr(amask),
                                                    _cabi.ptr(hidden), ws.data_ptr(), nbytes, _cabi.current_stream_handle(self.device),
                                                    self._status.data_ptr())
        _cabi.check(rc, "at_w2vbert_encode_checked")
        assert t_out.value == T
        if return_taps:
            return tokens, {"input_features": feats, "attention_mask": amask, "hidden": hidden}
        return tokens if want_tokens else hidden
