"""CPU: the host side of the streaming encode — AudioToken.stream refuses the non-causal tokenizers without touching a device, and
AcousticStream's residual buffering (pure host logic) hands the library whole frames only, holds the first push back until its minimum
is there, and sends the rest with final = True."""
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd.streaming import FIRST_PUSH_FRAMES, HOP, AcousticStream


@pytest.mark.parametrize("tok", [Tokenizers.semantic_m, Tokenizers.semantic_s])
def test_stream_is_acoustic_only(tok):
    at = AudioToken(tok, device="cuda:0")
    with pytest.raises(ValueError, match="acoustic"):
        at.stream()
    assert at.encoder is None, "the refusal must come before any model is loaded"


def test_encode_stream_needs_path_and_chunk_size():
    at = AudioToken(Tokenizers.acoustic, device="cuda:0")
    with pytest.raises(ValueError, match="chunk_size"):
        at.encode(torch.zeros(1, 24000), stream=True)
    assert at.encoder is None


class _Stub:
    """push_fn stand-in: records every library call and returns one id per frame that encodes the call's first sample position."""

    def __init__(self, B, n_q):
        self.calls, self.B, self.n_q, self.pos = [], B, n_q, 0
        self.seen = []

    def __call__(self, x, final):
        assert x.shape[0] == self.B and x.is_contiguous()
        n = x.shape[1]
        self.calls.append((n, final))
        self.seen.append(x.clone())
        t = -(-n // HOP)
        self.pos += n
        return torch.zeros(self.B, self.n_q, t, dtype=torch.int16)


def _run(sizes, B=2):
    stub = _Stub(B, 4)
    st = AcousticStream(None, B, push_fn=stub, n_q=4)
    total = sum(sizes)
    wav = torch.arange(B * total, dtype=torch.float32).reshape(B, total)
    outs, pos = [], 0
    for n in sizes:
        outs.append(st.push(wav[:, pos:pos + n]))
        pos += n
    outs.append(st.flush())
    return stub, st, wav, torch.cat(outs, dim=-1)


def test_residual_buffering_whole_frames_and_first_minimum():
    sizes = [100, 2000, 139, 1, 320, 7, 5000, 319]
    stub, st, wav, codes = _run(sizes)
    total = sum(sizes)
    assert codes.shape == (2, 4, -(-total // HOP)) and st.frames_emitted == codes.shape[-1]
    # every non-final call: a positive multiple of 320; the first one at least the minimum; exactly one final call, the last
    assert [f for _, f in stub.calls] == [False] * (len(stub.calls) - 1) + [True]
    assert all(n > 0 and n % HOP == 0 for n, f in stub.calls if not f)
    assert stub.calls[0][0] >= FIRST_PUSH_FRAMES * HOP
    assert stub.calls[-1][0] == total % HOP
    # nothing lost, duplicated or reordered
    assert torch.equal(torch.cat(stub.seen, dim=1), wav)
    # 100 + 2000 + 139 = 2239 samples: one short of the first push's minimum, the next sample releases 7 frames
    assert stub.calls[0] == (FIRST_PUSH_FRAMES * HOP, False)


def test_short_stream_is_one_final_call():
    stub, st, wav, codes = _run([300, 300, 300])
    assert stub.calls == [(900, True)] and codes.shape[-1] == 3


def test_frame_aligned_stream_flushes_nothing():
    stub, st, wav, codes = _run([3200, 3200])
    assert stub.calls == [(3200, False), (3200, False)] and codes.shape[-1] == 20


def test_push_after_flush_raises_until_reset():
    stub = _Stub(1, 2)
    st = AcousticStream(None, 1, push_fn=stub, n_q=2)
    st.push(torch.zeros(1, 3200))
    st.flush()
    with pytest.raises(RuntimeError):
        st.push(torch.zeros(1, 320))
    with pytest.raises(RuntimeError):
        st.flush()
    st.reset()
    assert st.frames_emitted == 0
    assert st.push(torch.zeros(1, 3200)).shape[-1] == 10


@pytest.mark.parametrize("first", [0, 10 * HOP], ids=["first_push", "after_whole_frames"])
def test_what_is_held_is_a_copy_of_the_callers_samples(first):
    """A caller may reuse the tensor it pushed: the end a stream holds back is its own copy, on the first push and after a push that left nothing held."""
    stub = _Stub(1, 4)
    st = AcousticStream(None, 1, push_fn=stub, n_q=4)
    if first:
        st.push(torch.zeros(1, first))
    buf = torch.arange(8 * HOP + 100, dtype=torch.float32)[None].clone()
    want = buf[:, -100:].clone()
    st.push(buf)
    buf.fill_(-1.0)                 # the caller's buffer goes on to other use
    st.flush()
    assert stub.calls[-1] == (100, True) and torch.equal(stub.seen[-1], want)
