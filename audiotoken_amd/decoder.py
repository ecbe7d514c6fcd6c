"""Decoder callable with the reference's protocol: ``decoder(tokens int64 [B, K, T]) -> float32 [1, B*320*T]``
(reference audiotoken/decoder.py:50-76), backed by libaudiotoken_hip.so. Only the acoustic decoder is in scope:
the semantic decoders (nanoGPT sampling + bark, decoder.py:79-245) are stochastic and need private weights."""
from __future__ import annotations

from typing import Dict, Optional, Union

import numpy as np
import torch

from . import _cabi, fallback
from . import weights as W
from .configs import AcousticDecoderConfig
from .encoder import _EncodecCallable


class AcousticDecoder(_EncodecCallable):
    """Drop-in for reference ``AcousticDecoder`` (audiotoken/decoder.py:50-76)."""

    def __init__(self, config: AcousticDecoderConfig = None, device: str = "cuda:0",
                 weights: Optional[Union[str, Dict[str, np.ndarray]]] = None):
        super().__init__()
        config = config or AcousticDecoderConfig()
        self.config = config
        self._open(device, weights if weights is not None else config.weights, with_decoder=True)

    def last_status(self) -> int:
        """0 = ok; bit 0 = a bounded wait inside the persistent LSTM kernel gave up; bit 1 = fp16 range overflow in an f16x2 kernel (LSTM input
        projection, residual blocks, transposed convs, tail). A decode has no quantiser, so bit 2 is never set. Synchronises the device."""
        return super().last_status()

    # the decoder's f16x2 kernel groups with a range check: LSTM input projection, residual blocks, transposed convs, fused tail
    RANGE_OPTIONS = ("ih_f16x2", "res_f16x2", "up_f16x2", "tail_f16x2")

    def verified(self, wav: torch.Tensor, tokens: torch.Tensor) -> torch.Tensor:
        """As AcousticEncoder.verified (fallback.encodec_ladder): on an LSTM hand-off time-out the LSTM route is switched for good, on an fp16 range
        overflow THIS batch is decoded again without the f16x2 kernels (``fallback_batches``); any status the repeat leaves raises."""
        return fallback.encodec_ladder(self, wav, lambda: self.forward(tokens), tokens.shape[0], self.RANGE_OPTIONS, "acoustic decode",
                                       nonfinite_bit=False)

    @torch.no_grad()
    def forward(self, input_batch: torch.Tensor) -> torch.Tensor:
        assert input_batch.dim() == 3, "tokens must be [B, K, T]"
        codes = input_batch.to(device=self.device, dtype=torch.long).contiguous()
        B, K, T = codes.shape
        lib = self._h.lib
        out = torch.empty((1, B * W.ENCODEC_HOP * T), dtype=torch.float32, device=self.device)
        nbytes = lib.at_encodec_decode_workspace_bytes(self._h.handle, B, T)
        ws = self._workspace(nbytes)
        with torch.cuda.device(self.device):
            rc = lib.at_encodec_decode_checked(self._h.handle, codes.data_ptr(), B, K, T, out.data_ptr(), ws.data_ptr(), nbytes,
                                               _cabi.current_stream_handle(self.device), self._status.data_ptr())
        _cabi.check(rc, "at_encodec_decode_checked")
        return out

    def new_stream(self, batch: int = 1):
        """A stateful decoder for tokens that arrive frame by frame (audiotoken_amd/streaming.py): the concatenated ``push`` outputs are the audio
        one-shot ``forward`` gives for the concatenated tokens, in memory bounded by the largest push. Streams of one decoder are independent."""
        from .streaming import AcousticDecodeStream
        return AcousticDecodeStream(self, batch)

    def new_stream_pool(self, slots: int = 1):
        """Up to ``slots`` decode streams that start and finish on their own (audiotoken_amd/streaming.py, AcousticDecodeStreamPool); the streams of
        one call with the same phase, K and number of frames share one library push."""
        from .streaming import AcousticDecodeStreamPool
        return AcousticDecodeStreamPool(self, slots)
