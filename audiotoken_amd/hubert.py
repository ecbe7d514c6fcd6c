"""semantic_s: ``HubertEncoder`` and ``hubert_processor`` with the reference's protocol
(audiotoken/encoder.py:20-26, 60-108), backed by libaudiotoken_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Union

import numpy as np
import torch

from . import _cabi, fallback
from . import weights as W
from ._handle import SemanticHandle
from .configs import HubertEncoderConfig
from .logger import get_logger

logger = get_logger(__name__)


def hubert_processor(audio: torch.Tensor, processor=None) -> torch.Tensor:
    """Reference ``hubert_processor`` (encoder.py:20-26) = HF ``Wav2Vec2FeatureExtractor(do_normalize=True)`` on one
    clip: zero mean / unit variance over the whole array, ``(x - mean) / sqrt(var + 1e-7)`` in float32. Host-side
    transform applied before batching, exactly where the reference applies it (core.py:188-189, datasets.py:78-79)."""
    x = np.asarray(audio, dtype=np.float32)
    y = (x - x.mean()) / np.sqrt(x.var() + 1e-7)
    return torch.from_numpy(y.astype(np.float32))


def fold_hubert_weights(w: Dict[str, np.ndarray], n_layers: int) -> Dict[str, np.ndarray]:
    out: Dict[str, np.ndarray] = {}
    for k, v in w.items():
        if k.startswith("encoder.layers.") and int(k.split(".")[2]) >= n_layers:
            continue   # layers past the consumed hidden state are dead compute
        if k.endswith("pos_conv_embed.conv.weight_g") or k.endswith("parametrizations.weight.original0"):
            base = k.rsplit(".", 1)[0] if k.endswith("weight_g") else k[: -len(".parametrizations.weight.original0")]
            vkey = base + ".weight_v" if k.endswith("weight_g") else base + ".parametrizations.weight.original1"
            folded = torch._weight_norm(torch.from_numpy(np.ascontiguousarray(w[vkey], dtype=np.float32)),
                                        torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)), 2)
            out["encoder.pos_conv_embed.conv.weight"] = folded.numpy()
        elif k.endswith("weight_v") or k.endswith("original1") or k == "masked_spec_embed":
            continue
        elif k == "kmeans.cluster_centers_":
            c = np.ascontiguousarray(v, dtype=np.float32)
            out[k] = c
            out["kmeans.c2"] = (torch.from_numpy(c) ** 2).sum(-1).numpy()
        else:
            out[k] = np.ascontiguousarray(v, dtype=np.float32)
    return out


HUBERT_ARCH = {"hidden_size": 768, "intermediate_size": 3072, "num_attention_heads": 12, "conv_dim": [512] * 7, "conv_kernel": [10, 3, 3, 3, 3, 2, 2],
               "conv_stride": [5, 2, 2, 2, 2, 2, 2], "conv_bias": False, "feat_extract_norm": "group", "do_stable_layer_norm": False,
               "num_conv_pos_embeddings": 128, "num_conv_pos_embedding_groups": 16, "hidden_act": "gelu"}


def load_hubert_checkpoint(model_dir: str, quantizer_path: Optional[str]) -> Dict[str, np.ndarray]:
    """The reference's ``HubertModel.from_pretrained`` directory (config.json + model.safetensors / pytorch_model.bin, possibly sharded,
    keys possibly under ``hubert.``) + the joblib k-means pickle whose ``cluster_centers_`` it reads (reference encoder.py:72, 84-85)."""
    sd = W.read_hf_state_dict(model_dir, strip_prefixes=("hubert.",))
    W.check_hf_config(model_dir, HUBERT_ARCH, "semantic_s checkpoint")
    if quantizer_path:
        import joblib
        sd["kmeans.cluster_centers_"] = np.asarray(joblib.load(quantizer_path).cluster_centers_, dtype=np.float32)
    return sd


class HubertEncoder(SemanticHandle, torch.nn.Module):
    """Drop-in for reference ``HubertEncoder`` (audiotoken/encoder.py:60-108)."""
    FAMILY, LAYER_NOUN = "hubert", "transformer"

    def __init__(self, config: HubertEncoderConfig = None, device: str = "cuda:0", quantize: bool = True,
                 weights: Optional[Union[str, Dict[str, np.ndarray]]] = None, packed=None):
        """``packed`` = ``(meta, blob)`` from another rank's ``export_packed()``: the finalized model is rebuilt over that device blob (``weights`` is ignored)."""
        super().__init__()
        config = config or HubertEncoderConfig()
        self.config = config
        self.quantize = quantize
        self.output_layer = config.output_layer
        self._create(device, packed, lambda: self._host_tensors(weights if weights is not None else config.weights))

    def _host_tensors(self, weights) -> Dict[str, np.ndarray]:
        if weights is None:
            logger.warning("No HuBERT checkpoint given (weights=/AUDIOTOKEN_HUBERT_WEIGHTS): synthetic weights, seed 0")
            weights = W.synth_hubert_weights(n_layers=self.output_layer, seed=0, with_kmeans=True)
        elif isinstance(weights, (str, bytes)):
            weights = load_hubert_checkpoint(weights, self.config.quantizer_path)
        return fold_hubert_weights(weights, self.output_layer)

    def site_scales(self):
        """[(scale of the q/k/v projection's input, scale of the first FFN GEMM's input) per transformer layer]: 16, or the provable scale of a LayerNorm
        whose gains are too large for 16 (include/audiotoken_hip.h, at_hubert_site_scales)."""
        buf = (C.c_float * 128)()
        n = self.lib.at_hubert_site_scales(self.handle, buf, 128)
        if n < 0:
            raise _cabi.HipLibraryError(f"at_hubert_site_scales failed: {_cabi.last_error()}")
        return [(float(buf[2 * l]), float(buf[2 * l + 1])) for l in range(n // 2)]

    def verified(self, tokens: torch.Tensor, input_batch: torch.Tensor, attention_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Product-path guard (see Wav2VecBertEncoder.verified): on an fp16 range overflow in a TRANSFORMER layer that layer moves to bf16x3 and the batch is
        repeated (the layer returns to f16x2 afterwards unless it was its PIN_AFTER-th overflowing batch); an overflow in the conv feature encoder / positional conv (a property of the input's level) repeats THIS batch with
        arith=bf16x3 for the whole model, then switches back."""
        return fallback.semantic_ladder(self, tokens, lambda: self.forward(input_batch, attention_mask), 1, self.LAYER_NOUN, "semantic_s encode")

    @torch.no_grad()
    def forward(self, input_batch: torch.Tensor, attention_mask: Optional[torch.Tensor] = None, n_layers: Optional[int] = None,
                return_hidden: bool = False):
        """``float32 [B, N]`` (normalised) + mask -> ``int16 [B, 1, T]`` on the device (hidden state if quantize=False)."""
        assert input_batch.dim() == 2, "input_batch must be [B, N]"
        x = input_batch.to(device=self.device, dtype=torch.float32).contiguous()
        m = None if attention_mask is None else attention_mask.to(device=self.device, dtype=torch.float32).contiguous()
        B, N = x.shape
        T = self.lib.at_hubert_num_tokens(N)
        nl = self.output_layer if n_layers is None else n_layers
        tokens = torch.empty((B, 1, T), dtype=torch.int16, device=self.device) if self.quantize else None
        hidden = torch.empty((B, T, 768), dtype=torch.float32, device=self.device) if (return_hidden or not self.quantize) else None
        nbytes = self.lib.at_hubert_workspace_bytes(self.handle, B, N)
        ws = self._workspace(nbytes)
        t_out = C.c_int(0)
        with torch.cuda.device(self.device):
            rc = self.lib.at_hubert_encode_checked(self.handle, x.data_ptr(), _cabi.ptr(m), B, N, nl, _cabi.ptr(tokens), C.byref(t_out),
                                                   _cabi.ptr(hidden), ws.data_ptr(), nbytes, _cabi.current_stream_handle(self.device),
                                                   self._status.data_ptr())
        _cabi.check(rc, "at_hubert_encode_checked")
        assert t_out.value == T
        if return_hidden:
            return tokens, hidden
        return tokens if self.quantize else hidden

    __call__ = torch.nn.Module.__call__   # the reference defines __call__ directly (encoder.py:87); same call protocol
