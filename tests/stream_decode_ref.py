"""CPU model of the streaming acoustic decode (AcousticDecodeStream / at_encodec_decode_stream_checked), restated over the oracle's own
primitives (oracle/encodec_ref.py: rvq_decode, conv1d_causal, convtr1d_causal, resblock) with the state-carrying LSTM of tests/stream_ref.py.

TEST INFRASTRUCTURE — never imported by the product path.

Per stream the carried state is: the last 6 rows of the quantised embedding z (the history of the k = 7 first conv), (h, c) of both LSTM
layers, the last CONTEXT_FRAMES rows of lstm(x0) + x0. A push gathers z for the new codes, runs the first conv over [6 carried rows | new rows]
without padding, continues the LSTM over the new rows, runs the upsampling stack on [context rows | new rows] and drops the context's
CONTEXT_FRAMES * 320 output samples (the window's zero / reflect left edge has touched only those). On the first push nothing is carried
and nothing is dropped: the left reflect padding is the true one.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

from oracle import encodec_ref as R
from tests.stream_ref import lstm_skip_state

HOP = 320
Z_HISTORY = 6            # rows of history of the first conv (k = 7)
FIRST_PUSH_FRAMES = 7    # a stream's first push holds at least this many frames, as one-shot decode does


def upsample_stack(w, y: torch.Tensor) -> torch.Tensor:
    """lstm + skip output [B, 512, T] -> waveform [B, 1, 320 T]: R.seanet_decode behind the LSTM."""
    x = y
    idx = 3
    for r in R.RATIOS_DEC:
        x = F.elu(x)
        p = f"decoder.model.{idx}.convtr.convtr"
        x = R.convtr1d_causal(x, R.folded(w, p), R._t(w, p + ".bias"), r)
        x = R.resblock(w, f"decoder.model.{idx + 1}", x)
        idx += 3
    x = F.elu(x)
    return R.conv1d_causal(x, R.folded(w, "decoder.model.15.conv.conv"), R._t(w, "decoder.model.15.conv.conv.bias"), 1)


class DecodeStreamModel:
    """The device algorithm on the CPU. push(tokens [B, K, t]) -> wav [B, 320 t]."""

    def __init__(self, w, batch: int = 1, context_frames: int = 2):
        self.w = w
        self.B = batch
        self.ctx_frames = context_frames
        self.reset()

    def reset(self):
        self.zhist: Optional[torch.Tensor] = None    # [B, 128, 6]; None = nothing consumed yet
        self.lstm = None
        self.yctx: Optional[torch.Tensor] = None     # [B, 512, ctx_frames]

    def push(self, tokens: torch.Tensor) -> torch.Tensor:
        B, K, t = tokens.shape
        assert B == self.B and t >= 1
        first = self.zhist is None
        z = R.rvq_decode(self.w, tokens.to(torch.long).transpose(0, 1))
        w0, b0 = R.folded(self.w, "decoder.model.0.conv.conv"), R._t(self.w, "decoder.model.0.conv.conv.bias")
        if first:
            assert t >= FIRST_PUSH_FRAMES, "the first push needs 7 frames, as one-shot decode does"
            x0 = R.conv1d_causal(z, w0, b0, 1)
            zwin = z
        else:
            zwin = torch.cat([self.zhist, z], dim=2)
            x0 = F.conv1d(zwin, w0, b0)   # no padding: the carried rows are the left context
        y, self.lstm = lstm_skip_state(self.w, "decoder.model.1", x0, self.lstm)
        ywin = y if first else torch.cat([self.yctx, y], dim=2)
        wav = upsample_stack(self.w, ywin)[:, 0, (0 if first else self.ctx_frames * HOP):]
        self.zhist = zwin[:, :, -Z_HISTORY:]
        self.yctx = ywin[:, :, ywin.shape[2] - self.ctx_frames:]
        return wav


def stream_decode(w, tokens: torch.Tensor, schedule: List[int], context_frames: int = 2) -> torch.Tensor:
    """tokens [B, K, T] pushed in pieces of the given frame counts (the rest in one last piece) -> wav [B, 320 T]."""
    m = DecodeStreamModel(w, tokens.shape[0], context_frames)
    outs, pos = [], 0
    for n in list(schedule) + [tokens.shape[2]]:
        if pos >= tokens.shape[2]:
            break
        outs.append(m.push(tokens[:, :, pos:pos + n]))
        pos += n
    return torch.cat(outs, dim=1)
