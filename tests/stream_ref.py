"""CPU model of the streaming acoustic encode (AcousticStream / at_encodec_encode_stream_checked), restated over the oracle's own
primitives (oracle/encodec_ref.py: conv1d_causal, resblock, rvq_encode) plus a local LSTM that takes and returns (h, c).

TEST INFRASTRUCTURE — never imported by the product path.

Per stream the carried state is: the last CONTEXT_FRAMES * 320 consumed samples, (h, c) of both LSTM layers, the last 6 rows of
ELU(lstm + skip) (the history of the final k = 7 conv). A push runs the conv stack on [context | new samples], drops the context's
output frames (reflect padding has touched them), runs the LSTM over the new frames from the carried state and the final conv over
[6 carried rows | new rows]. On the first push nothing is carried and nothing is dropped: the left reflect padding is the true one.
"""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn.functional as F

from oracle import encodec_ref as R

HOP = 320
FIN_HISTORY = 6          # rows of history of the final conv (k = 7)
FIRST_PUSH_FRAMES = 7    # a stream's first (non-final) push holds at least this many frames, as the device path does


def conv_stack(w, wav: torch.Tensor) -> torch.Tensor:
    """[B, N] -> the LSTM's input [B, 512, ceil(N/320)]: R.seanet_encode up to the stage-3 strided conv."""
    x = wav.unsqueeze(1)
    x = R.conv1d_causal(x, R.folded(w, "encoder.model.0.conv.conv"), R._t(w, "encoder.model.0.conv.conv.bias"), 1)
    idx = 1
    for r in R.RATIOS_ENC:
        x = R.resblock(w, f"encoder.model.{idx}", x)
        x = F.elu(x)
        p = f"encoder.model.{idx + 2}.conv.conv"
        x = R.conv1d_causal(x, R.folded(w, p), R._t(w, p + ".bias"), r)
        idx += 3
    return x


def lstm_skip_state(w, prefix: str, x: torch.Tensor, state):
    """R.lstm_skip with carried state: state = [(h, c), (h, c)] or None (zeros). Returns (lstm(x) + x, new state)."""
    B, C, T = x.shape
    seq = x.permute(2, 0, 1)
    inp = seq
    new_state = []
    for layer in range(2):
        w_ih = R._t(w, f"{prefix}.lstm.weight_ih_l{layer}")
        w_hh = R._t(w, f"{prefix}.lstm.weight_hh_l{layer}")
        b_ih = R._t(w, f"{prefix}.lstm.bias_ih_l{layer}")
        b_hh = R._t(w, f"{prefix}.lstm.bias_hh_l{layer}")
        H = w_hh.shape[1]
        if state is None:
            h = torch.zeros(B, H, dtype=x.dtype)
            c = torch.zeros(B, H, dtype=x.dtype)
        else:
            h, c = state[layer]
        outs = []
        xg = F.linear(inp, w_ih, b_ih)
        for t in range(T):
            gates = xg[t] + F.linear(h, w_hh, b_hh)
            i, f, g, o = gates.chunk(4, dim=1)
            c = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
            h = torch.sigmoid(o) * torch.tanh(c)
            outs.append(h)
        inp = torch.stack(outs, 0)
        new_state.append((h, c))
    return (inp + seq).permute(1, 2, 0), new_state


class StreamModel:
    """The device algorithm on the CPU. push(samples [B, n], final) -> emb [B, 128, t]; n is a multiple of 320 unless final."""

    def __init__(self, w, batch: int = 1, context_frames: int = 2):
        self.w = w
        self.B = batch
        self.ctx_len = context_frames * HOP
        self.ctx_frames = context_frames
        self.reset()

    def reset(self):
        self.ctx: Optional[torch.Tensor] = None      # [B, ctx_len]; None = nothing consumed yet
        self.lstm = None
        self.yhist: Optional[torch.Tensor] = None    # [B, 512, 6]
        self.finished = False

    def push(self, x: torch.Tensor, final: bool = False) -> torch.Tensor:
        assert not self.finished, "push after the final push"
        B, n = x.shape
        assert B == self.B
        assert final or n % HOP == 0
        first = self.ctx is None
        if n == 0:
            assert final
            self.finished = True
            return torch.zeros(B, 128, 0)
        if first:
            assert final or n >= max(FIRST_PUSH_FRAMES * HOP, self.ctx_len)
            window, drop = x, 0
        else:
            window, drop = torch.cat([self.ctx, x], dim=1), self.ctx_frames
        x4 = conv_stack(self.w, window)[:, :, drop:]
        y, self.lstm = lstm_skip_state(self.w, "encoder.model.13", x4, self.lstm)
        y = F.elu(y)
        wf, bf = R.folded(self.w, "encoder.model.15.conv.conv"), R._t(self.w, "encoder.model.15.conv.conv.bias")
        if first:
            emb = R.conv1d_causal(y, wf, bf, 1)
        else:
            emb = F.conv1d(torch.cat([self.yhist, y], dim=2), wf, bf)   # no padding: the carried rows are the left context
        if final:
            self.finished = True
        else:
            self.ctx = window[:, window.shape[1] - self.ctx_len:]
            self.yhist = torch.cat([self.yhist, y], dim=2)[:, :, -FIN_HISTORY:] if not first else y[:, :, -FIN_HISTORY:]
        return emb


class ResidualBuffer:
    """The host-side buffering of AcousticStream, restated: samples are held until a whole number of frames (and the first push's
    minimum) is there; flush() sends the rest with final = True."""

    def __init__(self, model: StreamModel):
        self.m = model
        self.held = torch.zeros(model.B, 0)

    def push(self, x: torch.Tensor) -> torch.Tensor:
        self.held = torch.cat([self.held, x], dim=1)
        n = self.held.shape[1] // HOP * HOP
        if n == 0 or (self.m.ctx is None and n < FIRST_PUSH_FRAMES * HOP):
            return torch.zeros(self.m.B, 128, 0)
        out = self.m.push(self.held[:, :n])
        self.held = self.held[:, n:]
        return out

    def flush(self) -> torch.Tensor:
        out = self.m.push(self.held, final=True)
        self.held = torch.zeros(self.m.B, 0)
        return out


def stream_encode(w, wav: torch.Tensor, schedule: List[int], context_frames: int = 2) -> torch.Tensor:
    """wav [B, N] pushed in pieces of the given sizes (any sizes; the rest in one last piece), then flushed -> emb [B, 128, ceil(N/320)]."""
    buf = ResidualBuffer(StreamModel(w, wav.shape[0], context_frames))
    outs, pos = [], 0
    for n in schedule:
        if pos >= wav.shape[1]:
            break
        outs.append(buf.push(wav[:, pos:pos + n]))
        pos += n
    if pos < wav.shape[1]:
        outs.append(buf.push(wav[:, pos:]))
    outs.append(buf.flush())
    return torch.cat(outs, dim=2)
