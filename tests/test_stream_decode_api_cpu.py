"""CPU: the host side of AcousticDecodeStream (holding tokens until the first push's 7 frames are there, flush / reset, the schedule sums)
with a stub in place of the device call, and the argument errors of AudioToken.decode_stream / decode(stream=True)."""
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd.streaming import FIRST_PUSH_FRAMES, HOP, AcousticDecodeStream


@pytest.mark.parametrize("tok", [Tokenizers.semantic_m, Tokenizers.semantic_s])
def test_decode_stream_is_acoustic_only(tok):
    at = AudioToken(tok, device="cuda:0")
    with pytest.raises(ValueError, match="acoustic"):
        at.decode_stream()
    assert at.decoder is None, "the refusal must come before any model is loaded"


def test_decode_stream_needs_chunk_size():
    at = AudioToken(Tokenizers.acoustic, device="cuda:0")
    with pytest.raises(ValueError, match="chunk_size"):
        at.decode(torch.zeros(1, 8, 75, dtype=torch.long), stream=True)
    assert at.decoder is None


class _Stub:
    """push_fn stand-in: records every library call and returns, per frame, 320 samples that hold the frame's first code of clip row b."""

    def __init__(self):
        self.calls = []

    def __call__(self, tokens):
        assert tokens.is_contiguous() and tokens.dim() == 3
        self.calls.append(tokens.shape[-1])
        return tokens[:, 0, :].to(torch.float32).repeat_interleave(HOP, dim=1)


def _tokens(B, K, T):
    # code of (b, k, t) = 1000 b + t for k = 0: the stub's output names the frame every sample came from
    t = torch.arange(T).view(1, 1, T) + 1000 * torch.arange(B).view(B, 1, 1)
    return t.expand(B, K, T).clone()


def _run(schedule, B=2, K=4):
    T = sum(schedule)
    toks = _tokens(B, K, T)
    stub = _Stub()
    st = AcousticDecodeStream(batch=B, push_fn=stub)
    outs, pos = [], 0
    for n in schedule:
        outs.append(st.push(toks[:, :, pos:pos + n]))
        pos += n
    return st, stub, toks, outs


def test_tokens_are_held_until_seven_frames():
    st, stub, toks, outs = _run([1, 2, 3, 1, 1, 5])
    assert [o.shape[1] for o in outs] == [0, 0, 0, HOP * FIRST_PUSH_FRAMES, HOP, 5 * HOP]
    assert stub.calls == [7, 1, 5]
    assert all(o.dtype == torch.float32 and o.shape[0] == 2 for o in outs)
    assert st.frames_emitted == 13


@pytest.mark.parametrize("schedule", ([7] + [1] * 20, [3, 3, 3, 10, 1, 40], [60], [9, 200, 1]))
def test_schedule_sums_and_order(schedule):
    st, stub, toks, outs = _run(schedule)
    wav = torch.cat(outs + [st.flush()], dim=1)
    T = sum(schedule)
    assert wav.shape == (2, HOP * T)
    assert torch.equal(wav, toks[:, 0, :].to(torch.float32).repeat_interleave(HOP, dim=1)), "every frame once, in order"
    assert sum(stub.calls) == T and st.frames_emitted == T
    assert stub.calls[0] >= FIRST_PUSH_FRAMES


def test_flush_on_a_started_stream_returns_nothing():
    st, stub, toks, outs = _run([8, 2])
    n = len(stub.calls)
    out = st.flush()
    assert out.shape == (2, 0) and len(stub.calls) == n


def test_flush_sends_what_a_never_started_stream_holds():
    st, stub, toks, outs = _run([2, 3])
    assert stub.calls == []
    out = st.flush()   # 5 frames: the device call would refuse them as one-shot decode refuses T = 5; the stub shows they are all sent
    assert stub.calls == [5] and out.shape == (2, 5 * HOP)


def test_push_after_flush_raises_until_reset():
    st, stub, toks, outs = _run([7])
    st.flush()
    with pytest.raises(RuntimeError, match="after flush"):
        st.push(toks[:, :, :1])
    with pytest.raises(RuntimeError, match="twice"):
        st.flush()
    st.reset()
    assert st.frames_emitted == 0
    assert st.push(toks[:, :, :3]).shape == (2, 0)        # a new stream holds tokens again
    assert st.push(toks[:, :, 3:7]).shape == (2, 7 * HOP)
    assert stub.calls == [7, 7]


def test_batch_is_checked():
    st = AcousticDecodeStream(batch=2, push_fn=_Stub())
    with pytest.raises(AssertionError):
        st.push(_tokens(3, 4, 7))
