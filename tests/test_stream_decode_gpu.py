"""GPU: the streaming acoustic decode (AcousticDecodeStream / at_encodec_decode_stream_checked) against the CPU oracle and against the one-shot
decode of the same handle and options.

The bar.
* The oracle bar is asserted in EVERY case: against R.acoustic_decode of the same tokens, max-abs < 1e-3 and relative L2 < 1e-4 (what
  tests/test_acoustic_gpu.py::test_decode_matches_golden asks of one-shot decode). Weights: seed 0, family "trained_like".
* One-shot decode is unchanged by the streaming work and is the yardstick. Where a push and one-shot select the same kernels the outputs are
  asserted torch.equal: that is a stream's FIRST push (any B, K, t >= 7; schedule "one_push" and the first piece of every other schedule),
  which is a one-shot decode of its frames that also writes the state — under every option but "lstm_f16x2" = 0, where a push runs the fp32
  persistent recurrence because the three-piece bf16 kernel has no state variant. Later pushes run the same arithmetic on other tiles (the window's tile
  boundaries select the GEMM's interior or boundary body, the projection GEMM of the LSTM sees another M, a 1-frame window is 3 rows): for them
  only the oracle bar applies; their difference to one-shot is printed, not bounded by a number taken from the code under test.
* T > 1 500 (the 22 500-frame clip): a full CPU decode is too slow for a GPU session, so the oracle is evaluated on TWO WINDOWS, the first
  300 frames (exact: the decoder is causal, a prefix of the decode is the decode of the prefix) and the last 300 frames (the oracle's
  first conv and LSTM over all frames, its upsampling stack over the last 302 rows with the first 640 samples dropped: the receptive field
  argued in tests/stream_decode_ref.py and checked by tests/test_stream_decode_model_cpu.py).
"""
import functools

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.streaming import HOP
from oracle import encodec_ref as R
from tests.stream_decode_ref import upsample_stack

pytestmark = pytest.mark.gpu

ABS_BAR, REL_BAR = 1e-3, 1e-4     # test_decode_matches_golden's


@pytest.fixture(scope="module")
def dec_weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True, family="trained_like")


def _decoder(weights):
    from audiotoken_amd.configs import AcousticDecoderConfig
    from audiotoken_amd.decoder import AcousticDecoder
    return AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=weights)


@pytest.fixture(scope="module")
def decoder(cuda_device, dec_weights):
    return _decoder(dec_weights)


@functools.lru_cache(maxsize=None)
def _tokens(B, K, T, seed=0):
    return torch.randint(0, 1024, (B, K, T), dtype=torch.long, generator=torch.Generator().manual_seed(7000 + 131 * B + 17 * K + T + seed))


def _random_schedule(total, seed, hi=200):
    rng = np.random.default_rng(seed)
    out = [int(rng.integers(7, hi + 1))]
    while sum(out) < total:
        out.append(int(rng.integers(1, hi + 1)))
    return out


SCHEDULES = {
    "one_push": lambda T: [T],
    "seven_then_single": lambda T: [7] + [1] * (T - 7),
    "frames_75": lambda T: [75] * (T // 75 + 1),
    "random": lambda T: _random_schedule(T, 11),
}

_ORACLE = {}


def _oracle(weights, B, K, T):
    if (B, K, T) not in _ORACLE:
        _ORACLE[(B, K, T)] = R.acoustic_decode(weights, _tokens(B, K, T)).reshape(B, HOP * T)
    return _ORACLE[(B, K, T)]


def _one_shot(dec, toks):
    wav = dec(toks.cuda())
    assert dec.last_status() == 0
    return wav.reshape(toks.shape[0], -1).clone()


def _streamed(dec, toks, schedule, stream=None):
    """toks [B, K, T] pushed in pieces of the given frame counts, then flushed -> (wav [B, 320 T] on the device, per-piece outputs)."""
    st = stream if stream is not None else dec.new_stream(toks.shape[0])
    dev = toks.cuda()
    parts, pos = [], 0
    for n in schedule:
        if pos >= toks.shape[2]:
            break
        parts.append(st.push(dev[:, :, pos:pos + n]).clone())
        pos += n
    parts.append(st.flush())
    assert dec.last_status() == 0
    return torch.cat(parts, dim=1), parts


def _assert_bar(got, ref, what):
    got, ref = got.cpu().double(), ref.double()
    err = (got - ref).abs().max().item()
    rel = ((got - ref).norm() / ref.norm()).item()
    print(f"{what}: max abs err {err:.3e}, relative L2 {rel:.3e} at waveform scale {ref.abs().max().item():.2f}")
    assert err < ABS_BAR and rel < REL_BAR, f"{what}: max abs {err}, relative L2 {rel}"


CASES = ([(8, 1, 150, s) for s in SCHEDULES] + [(2, 1, 150, "random")] +
         [(2, 3, 150, s) for s in ("one_push", "seven_then_single", "frames_75", "random")] + [(8, 3, 90, "random")] +
         [(8, 64, 40, s) for s in ("one_push", "seven_then_single", "random")] + [(2, 64, 80, "frames_75")])


@pytest.mark.parametrize("K,B,T,schedule", CASES)
def test_stream_matches_oracle_and_one_shot(decoder, dec_weights, K, B, T, schedule):
    toks = _tokens(B, K, T)
    sched = SCHEDULES[schedule](T) if schedule != "random" else _random_schedule(T, 11, hi=min(200, max(8, T // 3)))
    wav, parts = _streamed(decoder, toks, sched)
    assert wav.dtype == torch.float32 and tuple(wav.shape) == (B, HOP * T)
    what = f"K={K} B={B} T={T} {schedule}"
    _assert_bar(wav, _oracle(dec_weights, B, K, T), what)
    one = _one_shot(decoder, toks)
    first = sched[0]
    # the first push is a one-shot decode of its frames: same kernels, same bits
    assert torch.equal(parts[0], _one_shot(decoder, toks[:, :, :first])), f"{what}: the first push differs from one-shot decode of its frames"
    if schedule == "one_push":
        assert torch.equal(wav, one), f"{what}: one push differs from one-shot decode"
    else:
        print(f"{what}: max |stream - one-shot| {(wav - one).abs().max().item():.3e} (not bounded: other kernels' tiles, see the header)")


def _oracle_suffix(weights, toks, n):
    """The oracle's last n frames of audio [B, 320 n] without decoding the whole clip at 24 kHz (header comment)."""
    z = R.rvq_decode(weights, toks.transpose(0, 1))
    x = R.conv1d_causal(z, R.folded(weights, "decoder.model.0.conv.conv"), R._t(weights, "decoder.model.0.conv.conv.bias"), 1)
    y = R.lstm_skip(weights, "decoder.model.1", x)
    return upsample_stack(weights, y[:, :, -(n + 2):])[:, 0, 2 * HOP:]


LONG_T, WINDOW = 22500, 300


@pytest.fixture(scope="module")
def long_oracle(dec_weights):
    toks = _tokens(1, 8, LONG_T)
    return R.acoustic_decode(dec_weights, toks[:, :, :WINDOW]).reshape(1, -1), _oracle_suffix(dec_weights, toks, WINDOW)


@pytest.mark.parametrize("schedule", ("frames_75", "random"))
def test_long_clip_against_oracle_windows(decoder, long_oracle, schedule):
    """B = 1, K = 8, 22 500 frames (300 s). Oracle on a prefix and a suffix window of 300 frames each (header comment)."""
    toks = _tokens(1, 8, LONG_T)
    wav, parts = _streamed(decoder, toks, SCHEDULES[schedule](LONG_T))
    assert tuple(wav.shape) == (1, HOP * LONG_T)
    prefix, suffix = long_oracle
    _assert_bar(wav[:, :HOP * WINDOW], prefix, f"T={LONG_T} {schedule}, first {WINDOW} frames")
    _assert_bar(wav[:, -HOP * WINDOW:], suffix, f"T={LONG_T} {schedule}, last {WINDOW} frames")
    one = _one_shot(decoder, toks)
    print(f"T={LONG_T} {schedule}: max |stream - one-shot| over the whole clip {(wav - one).abs().max().item():.3e}")
    _assert_bar(one[:, -HOP * WINDOW:], suffix, f"T={LONG_T} one-shot, last {WINDOW} frames")


# every LSTM route and every decoder option one-shot decode can take; B = 96 leaves the pipelined launch's 80-clip limit
ROUTES = [({"persistent_lstm": 0}, 3), ({"lstm_pipe": 0}, 3), ({"lstm_x3": 0}, 3), ({"lstm_f16x2": 0}, 3), ({"lstm_f16x2": 1}, 96),
          ({"lstm_f16x2": 0}, 96), ({"fused_dectail": 0}, 3), ({"fused_dectail": 1, "tail_f16x2": 0}, 3), ({"dec_chain": 0}, 3), ({"up_f16x2": 0}, 3),
          ({"res_f16x2": 0}, 3), ({"tail_f16x2": 0}, 1), ({"ih_f16x2": 0, "res_f16x2": 0, "up_f16x2": 0, "tail_f16x2": 0}, 3), ({"subbatch": 2}, 5)]


@pytest.mark.parametrize("options,B", ROUTES, ids=[",".join(f"{k}={v}" for k, v in o.items()) + f",B={b}" for o, b in ROUTES])
def test_every_route_carries_state(cuda_device, dec_weights, options, B):
    """1-frame pushes (3-row windows), a 2-frame and longer ones on every kernel route; the first push equals one-shot under the same options
    (except with "lstm_f16x2" = 0, where a push falls back to the fp32 recurrence)."""
    dec = _decoder(dec_weights)
    for k, v in options.items():
        dec.set_option(k, v)
        assert dec.get_option(k) == v
    K, T = 8, 36
    toks = _tokens(B, K, T, seed=1)
    sched = [9, 1, 1, 2, 1, 5, 17]
    wav, parts = _streamed(dec, toks, sched)
    _assert_bar(wav, R.acoustic_decode(dec_weights, toks).reshape(B, -1), f"{options} B={B}")
    first = _one_shot(dec, toks[:, :, :sched[0]])
    if options.get("lstm_f16x2", 1) == 0:
        # the three-piece bf16 recurrence has no state variant: a push runs the fp32 persistent kernel where one-shot runs the bf16 one (header of
        # include/audiotoken_hip.h) — other kernels, so only the oracle bar applies
        print(f"{options} B={B}: first push, max |stream - one-shot| {(parts[0] - first).abs().max().item():.3e}")
    else:
        assert torch.equal(parts[0], first)
    print(f"{options} B={B}: max |stream - one-shot| {(wav - _one_shot(dec, toks)).abs().max().item():.3e}")


@pytest.mark.parametrize("options", ({}, {"tail_f16x2": 0}, {"fused_dectail": 0}), ids=("dectail_x2", "dectail_f32", "conv_last"))
def test_skip_variant_with_skip_zero_is_the_stateless_kernel(cuda_device, dec_weights, options):
    """Option "dec_skip_twin": one-shot decode stores through the skip / stride variant of the tail kernel with skip = 0 and a dense stride."""
    dec = _decoder(dec_weights)
    for k, v in options.items():
        dec.set_option(k, v)
    toks = _tokens(3, 8, 45, seed=2)
    plain = _one_shot(dec, toks)
    dec.set_option("dec_skip_twin", 1)
    assert dec.get_option("dec_skip_twin") == 1
    twin = _one_shot(dec, toks)
    assert torch.equal(plain, twin)
    _assert_bar(twin, R.acoustic_decode(dec_weights, toks).reshape(3, -1), f"skip twin {options}")


def test_long_file_decode_in_one_chunks_memory(cuda_device, dec_weights, tmp_path):
    """AudioToken.decode(path, chunk_size=10, stream=True) = the per-push concatenation, in the workspace of one 750-frame push."""
    from audiotoken_amd import AudioToken, Tokenizers
    T = 3000 + 123
    toks = _tokens(1, 8, T, seed=3)
    path = tmp_path / "tokens.pt"
    torch.save(toks, path)
    tok = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=8, weights=dec_weights)
    audio = tok.decode(path, chunk_size=10, stream=True)
    assert audio.device.type == "cpu" and tuple(audio.shape) == (1, HOP * T)
    dec = tok.decoder
    lib, h = dec._h.lib, dec._h.handle
    per_push = lib.at_encodec_decode_stream_workspace_bytes(h, 1, 750)
    whole = lib.at_encodec_decode_workspace_bytes(h, 1, T)
    print(f"workspace: one 750-frame push {per_push / 2**20:.1f} MiB, one-shot decode of {T} frames {whole / 2**20:.1f} MiB")
    assert dec._ws.numel() == per_push, "the streamed decode's peak workspace is that of one 750-frame push"
    assert per_push < whole
    wav, _ = _streamed(dec, toks, [750] * 5)
    assert torch.equal(audio, wav.cpu())
    _assert_bar(audio[:, :HOP * 300], R.acoustic_decode(dec_weights, toks[:, :, :300]).reshape(1, -1), "streamed file decode, first 300 frames")
    # without stream=True decode is what it was
    assert torch.equal(tok.decode(toks[:, :, :40]), _one_shot(dec, toks[:, :, :40]).cpu().reshape(1, -1))


def test_single_frame_push_is_real_time(decoder):
    """75 frames per second leave 13.33 ms per frame: the median wall time of a 1-frame push (B = 1, the status read included) is below that."""
    import time
    toks = _tokens(1, 8, 7 + 50 + 256, seed=4).cuda()
    st = decoder.new_stream(1)
    st.push(toks[:, :, :7])
    for t in range(7, 57):   # warm-up
        st.push(toks[:, :, t:t + 1])
    torch.cuda.synchronize()
    times = []
    for t in range(57, 57 + 256):
        t0 = time.perf_counter()
        out = st.push(toks[:, :, t:t + 1])   # returns after the status word was read: the audio is complete
        times.append(time.perf_counter() - t0)
    assert tuple(out.shape) == (1, HOP)
    med = float(np.median(times)) * 1e3
    print(f"1-frame push, B = 1: median {med:.3f} ms, p90 {float(np.percentile(times, 90)) * 1e3:.3f} ms over {len(times)} pushes")
    assert med < 1000.0 / 75.0


def test_flush_below_seven_frames_raises_what_one_shot_raises(decoder):
    from audiotoken_amd._cabi import HipLibraryError
    toks = _tokens(1, 8, 5, seed=5).cuda()
    with pytest.raises(HipLibraryError):
        decoder(toks)
    st = decoder.new_stream(1)
    assert st.push(toks).shape == (1, 0)
    with pytest.raises(HipLibraryError, match="7 frames"):
        st.flush()
    st.reset()   # and the stream object is usable again
    more = _tokens(1, 8, 9, seed=6)
    assert torch.equal(st.push(more), _one_shot(decoder, more))
