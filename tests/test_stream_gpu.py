"""GPU: the streaming acoustic encode (AcousticStream / at_encodec_encode_stream_checked) against the one-shot encode of the same handle and
against the CPU oracle.

The bar. One-shot encode is unchanged by the streaming work and is itself oracle-checked, so it is the yardstick.
* Where one-shot and the pushes select the same kernels — a total length that is a multiple of 320, pushed in whole frames — embeddings and
  codes are asserted torch.equal (measured: profiles/stream_encode.txt; include/audiotoken_hip.h states it as the contract).
* An odd total, or one whose stage-1 length is not a multiple of 4, makes the one-shot call take other kernels than the mid-stream windows do
  ("same tokens, embeddings differ in the last bits"): codes equal one-shot's, embeddings and ids are held to the oracle bar.
* The oracle bar (tests/parity.py: embeddings within FLOAT_TOL, ids equal or explained by an oracle near-tie) is asserted in every case.
"""
import functools

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from oracle import encodec_ref as R
from tests import parity as P

pytestmark = pytest.mark.gpu

HOP = 320
FRAMES = 45
RANGE_OPTIONS = ("ih_f16x2", "chain_f16x2", "res_f16x2", "rvq_f16x2", "fin_f16x2")


@pytest.fixture(scope="module")
def enc_weights():
    return W.synth_encodec_weights(seed=0, with_decoder=False)


def _encoder(weights, n_q=8):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    return AcousticEncoder(AcousticEncoderConfig(bandwidth={2: 1.5, 4: 3, 8: 6}[n_q]), device="cuda:0", weights=weights)


@pytest.fixture(scope="module")
def encoders(cuda_device, enc_weights):
    return {nq: _encoder(enc_weights, nq) for nq in (2, 8)}


def _random_schedule(total, seed):
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < total:
        n = int(rng.integers(1, 4000))
        out.append(n)
        pos += n
    return out


SCHEDULES = {
    "one_push": lambda total: [total],
    "hop_320": lambda total: [320] * (total // 320 + 1),
    "hop_6400": lambda total: [6400] * (total // 6400 + 1),
    "random": lambda total: _random_schedule(total, 11),
}


@functools.lru_cache(maxsize=None)
def _wav(B, total, seed=None):
    return torch.from_numpy(W.synth_waveform(B, total, 24000, seed=1000 + B if seed is None else seed))


_ORACLE = {}


def _oracle(weights, B, total, n_q, seed=None):
    key = (B, total, n_q, seed)
    if key not in _ORACLE:
        wav = _wav(B, total, seed)
        emb = R.seanet_encode(weights, wav)
        codes, margins = R.rvq_encode(weights, emb, n_q, return_margins=True)
        _ORACLE[key] = (emb.permute(0, 2, 1).contiguous(), codes.transpose(0, 1).to(torch.int16), margins.transpose(0, 1))
    return _ORACLE[key]


def _one_shot(enc, x):
    codes, emb = enc(x, None, return_embeddings=True)
    assert enc.last_status() == 0
    return codes.clone(), emb.clone()


def _streamed(enc, x, schedule, stream=None):
    """x [B, N] on the device pushed in pieces of the given sizes, then flushed -> (codes [B, n_q, T], emb [B, T, 128], library calls)."""
    st = stream if stream is not None else enc.new_stream(x.shape[0])
    st.keep_embeddings = True
    codes, embs, pos, calls = [], [], 0, 0

    def take(c):
        nonlocal calls
        if c.shape[-1] > 0:
            codes.append(c.clone())
            embs.append(st.last_embeddings.clone())
            calls += 1

    for n in schedule:
        if pos >= x.shape[1]:
            break
        take(st.push(x[:, pos:pos + n]))
        pos += n
    if pos < x.shape[1]:
        take(st.push(x[:, pos:]))
    take(st.flush())
    assert enc.last_status() == 0
    return torch.cat(codes, dim=-1), torch.cat(embs, dim=1), calls


def _assert_oracle_bar(weights, codes, emb, B, total, n_q, what, seed=None):
    emb_ref, codes_ref, margins = _oracle(weights, B, total, n_q, seed)
    err = (emb.cpu() - emb_ref).abs().max().item()
    print(f"{what}: max |stream - oracle| embedding difference {err:.3e}")
    assert err < P.FLOAT_TOL, f"{what}: embedding differs from the oracle by {err}"
    P.assert_rvq_equal_or_explained(codes.cpu(), codes_ref, margins, P.RVQ_TIE, what)


def _same_kernels(total):
    """One-shot of `total` samples and frame-aligned windows select the same kernels: even length, stage lengths divisible by 4 / 5 / 8."""
    return total % HOP == 0


def _check_against_one_shot(enc, weights, B, total, n_q, schedule, what, seed=None):
    x = _wav(B, total, seed).cuda()
    c1, e1 = _one_shot(enc, x)
    cs, es, calls = _streamed(enc, x, schedule)
    assert cs.shape == c1.shape == (B, n_q, -(-total // HOP)) and es.shape == e1.shape
    diff = (es - e1).abs().max().item()
    print(f"{what}: {calls} library pushes, max |stream - one-shot| embedding difference {diff:.3e}")
    assert torch.equal(cs, c1), f"{what}: {int((cs != c1).sum())} token ids differ from one-shot"
    if _same_kernels(total):
        assert torch.equal(es, e1), f"{what}: embeddings differ from one-shot by {diff}"
    _assert_oracle_bar(weights, cs, es, B, total, n_q, what, seed)
    return calls


# ---- 3. stream vs one-shot ------------------------------------------------------------------------------------------------------------
# tails: 0 (all kernels shared), 1 / 9 / 319 (odd or ragged totals: fused stage 0 needs an even N), 2 (even, but the stage-1 length 7201 is
# not a multiple of 4 for the whole clip while it is for every mid-stream window)
CASES = [(1, 8, s, t) for s in sorted(SCHEDULES) for t in (0, 1, 2, 9, 319)]
CASES += [(3, 2, "random", 0), (3, 2, "hop_6400", 9), (3, 8, "hop_320", 0), (3, 2, "one_push", 319)]
CASES += [(17, 8, "hop_320", 0), (17, 8, "random", 319), (17, 2, "hop_6400", 2)]
CASES += [(81, 2, "hop_6400", 0), (81, 8, "random", 1), (81, 2, "hop_320", 0)]


@pytest.mark.parametrize("B,n_q,schedule,tail", CASES)
def test_stream_equals_one_shot(encoders, enc_weights, B, n_q, schedule, tail):
    total = FRAMES * HOP + tail
    calls = _check_against_one_shot(encoders[n_q], enc_weights, B, total, n_q, SCHEDULES[schedule](total), f"B {B}, n_q {n_q}, {schedule}, tail {tail}")
    if schedule != "one_push":
        assert calls > 1


# ---- 4. every LSTM route and the safe kernels --------------------------------------------------------------------------------------------
ROUTES = {
    "lstm_pipe=0": {"lstm_pipe": 0},
    "persistent_lstm=0": {"persistent_lstm": 0},
    "lstm_x3=0": {"lstm_x3": 0},
    "range_options=0": {o: 0 for o in RANGE_OPTIONS},
    "range_options=0,persistent_lstm=0": dict({o: 0 for o in RANGE_OPTIONS}, persistent_lstm=0),
}


@pytest.mark.parametrize("B", [3, 81])
@pytest.mark.parametrize("route", sorted(ROUTES))
def test_stream_on_every_route(enc_weights, cuda_device, route, B):
    enc = _encoder(enc_weights, 8)
    for k, v in ROUTES[route].items():
        enc.set_option(k, v)
    for tail, schedule in ((0, "hop_6400"), (9, "random")):
        total = FRAMES * HOP + tail
        _check_against_one_shot(enc, enc_weights, B, total, 8, SCHEDULES[schedule](total), f"{route}, B {B}, {schedule}, tail {tail}")


def test_three_piece_recurrence_streams_on_the_fp32_kernel(enc_weights, cuda_device):
    """"lstm_f16x2" = 0 selects the three-piece bf16 recurrence, which has no state variant (no registers left): a push then runs the fp32
    persistent kernel. One-shot under the same option rounds differently in the last bits, so this twin is held to equal codes and the oracle bar."""
    enc = _encoder(enc_weights, 8)
    enc.set_option("lstm_f16x2", 0)
    enc.set_option("lstm_pipe", 0)
    total = FRAMES * HOP
    x = _wav(3, total).cuda()
    c1, _ = _one_shot(enc, x)
    cs, es, _ = _streamed(enc, x, SCHEDULES["hop_6400"](total))
    assert torch.equal(cs, c1)
    _assert_oracle_bar(enc_weights, cs, es, 3, total, 8, "lstm_f16x2 = 0")


def test_route_change_in_mid_stream(enc_weights, cuda_device):
    """Pipelined -> layer-by-layer -> per-step launches between pushes of ONE stream: the state is route independent. The per-step LSTM is fp32 and
    differs from the persistent one in the last bits, so the oracle bar only."""
    enc = _encoder(enc_weights, 8)
    total = FRAMES * HOP + 9
    x = _wav(3, total).cuda()
    st = enc.new_stream(3)
    st.keep_embeddings = True
    codes, embs = [], []
    for i, (a, b) in enumerate(((0, 3200), (3200, 6400), (6400, 9600), (9600, 12800), (12800, total))):
        if i == 1:
            enc.set_option("lstm_pipe", 0)
        if i == 2:
            enc.set_option("persistent_lstm", 0)
        if i == 3:
            enc.set_option("persistent_lstm", 1)
            enc.set_option("lstm_x3", 0)
        if i == 4:
            enc.set_option("lstm_x3", 1)
            enc.set_option("lstm_pipe", 1)
        c = st.push(x[:, a:b])
        if c.shape[-1]:
            codes.append(c.clone()); embs.append(st.last_embeddings.clone())
    c = st.flush()
    codes.append(c.clone()); embs.append(st.last_embeddings.clone())
    _assert_oracle_bar(enc_weights, torch.cat(codes, -1), torch.cat(embs, 1), 3, total, 8, "route change in mid-stream")


# ---- 5. transactions ------------------------------------------------------------------------------------------------------------------
def test_forced_timeout_in_mid_stream_is_repeated_from_the_input_state(enc_weights, cuda_device):
    """lstm_spin_limit = 0 makes one push report status 1; the stream repeats it from the unchanged input state on another LSTM route. The whole
    token sequence equals the undisturbed stream's."""
    B, total = 20, FRAMES * HOP
    x = _wav(B, total).cuda()
    pieces = [(0, 4800), (4800, 9600), (9600, total)]
    ref_enc = _encoder(enc_weights, 8)
    ref, _, _ = _streamed(ref_enc, x, [b - a for a, b in pieces])
    enc = _encoder(enc_weights, 8)
    st = enc.new_stream(B)
    out = [st.push(x[:, 0:4800]).clone()]
    enc.set_option("lstm_spin_limit", 0)
    probe = st._call(x[:, 4800:9600].contiguous(), False)     # the bare library call: must report the give-up and leave the input state alone
    assert enc.last_status() == 1, "a give-up must be visible in the status word"
    del probe
    out.append(st.push(x[:, 4800:9600]).clone())              # status 1 again -> route switched -> repeated from the same input state
    assert enc.last_status() == 0
    assert enc.get_option("lstm_pipe") == 0
    enc.set_option("lstm_spin_limit", 1 << 18)
    out.append(st.push(x[:, 9600:]).clone())
    out.append(st.flush().clone())
    got = torch.cat(out, -1)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} ids differ from the undisturbed stream"
    _, codes_ref, margins = _oracle(enc_weights, B, total, 8)
    P.assert_rvq_equal_or_explained(got.cpu(), codes_ref, margins, P.RVQ_TIE, "stream with a forced hand-off timeout")


def test_loud_push_falls_back_for_that_push_only(enc_weights, cuda_device):
    """One push whose first third is 3e4 times louder overflows the fp16 range (status bit 1): it is repeated on the bf16x3 kernels from the
    unchanged state, counted once, and the next push runs on f16x2 again. Reference: a stream that is TOLD to take the safe kernels for that push."""
    B, total = 3, FRAMES * HOP
    wav = _wav(B, total, seed=77).clone()
    # loud for 5 frames; the push's last 10 frames are quiet again, so everything the next push inherits is in range: its 640 context samples and
    # the final conv's 6 history rows (frames 24..29, which reach back to sample 24 * 320 - 478 = 7202)
    wav[:, 4800:6400] *= 3e4
    x = wav.cuda()
    ref_enc = _encoder(enc_weights, 8)
    rs = ref_enc.new_stream(B)
    ref = [rs.push(x[:, 0:4800]).clone()]
    for o in RANGE_OPTIONS:
        ref_enc.set_option(o, 0)
    ref.append(rs.push(x[:, 4800:9600]).clone())
    for o in RANGE_OPTIONS:
        ref_enc.set_option(o, 1)
    ref.append(rs.push(x[:, 9600:]).clone())
    ref.append(rs.flush().clone())
    assert ref_enc.fallback_batches == 0
    enc = _encoder(enc_weights, 8)
    st = enc.new_stream(B)
    out = [st.push(x[:, 0:4800]).clone()]
    probe = st._call(x[:, 4800:9600].contiguous(), False)
    assert enc.last_status() & 2, "the range overflow was not reported"
    del probe
    before = {o: enc.get_option(o) for o in RANGE_OPTIONS}
    out.append(st.push(x[:, 4800:9600]).clone())
    assert enc.fallback_batches == 1 and st.fallback_batches == 1
    assert {o: enc.get_option(o) for o in RANGE_OPTIONS} == before, "the range fallback must not outlive the push"
    out.append(st.push(x[:, 9600:]).clone())
    assert enc.last_status() == 0 and enc.fallback_batches == 1, "the push after the loud one must run on f16x2 again (no second repeat)"
    assert all(enc.get_option(o) == 1 for o in RANGE_OPTIONS)
    out.append(st.flush().clone())
    got, want = torch.cat(out, -1), torch.cat(ref, -1)
    assert torch.equal(got, want), f"{int((got != want).sum())} ids differ from the stream that was told to use the safe kernels"
    codes_ref, margins = R.acoustic_encode(enc_weights, wav, 8, return_margins=True)
    P.assert_rvq_equal_or_explained(got.cpu(), codes_ref, margins, P.RVQ_TIE, "stream with one loud push")


# ---- 6. independence ------------------------------------------------------------------------------------------------------------------
def test_two_streams_on_one_encoder_and_reset(encoders, enc_weights):
    enc = encoders[8]
    total = FRAMES * HOP + 9
    xa, xb = _wav(2, total, seed=5).cuda(), _wav(2, total, seed=6).cuda()
    sched = SCHEDULES["random"](total)
    ca, ea, _ = _streamed(enc, xa, sched)
    cb, eb, _ = _streamed(enc, xb, sched)
    sa, sb = enc.new_stream(2), enc.new_stream(2)
    oa, ob, pos = [], [], 0
    for n in sched:
        oa.append(sa.push(xa[:, pos:pos + n]).clone())
        ob.append(sb.push(xb[:, pos:pos + n]).clone())
        pos += n
    oa.append(sa.flush().clone())
    ob.append(sb.flush().clone())
    assert torch.equal(torch.cat(oa, -1), ca) and torch.equal(torch.cat(ob, -1), cb)
    # after reset() a stream repeats its first run exactly
    sa.reset()
    assert sa.frames_emitted == 0
    c2, e2, _ = _streamed(enc, xa, sched, stream=sa)
    assert torch.equal(c2, ca) and torch.equal(e2, ea)
    assert sa.frames_emitted == ca.shape[-1]


# ---- 7. bounded memory ----------------------------------------------------------------------------------------------------------------
def test_five_minutes_in_ten_second_pushes(encoders, enc_weights):
    enc = encoders[8]
    lib, h = enc._h.lib, enc._h.handle
    n_push, pushes = 240000, 30
    total = n_push * pushes                      # 300 s, 22 500 frames
    state = lib.at_encodec_stream_state_bytes(h, 1)
    need = lib.at_encodec_stream_workspace_bytes(h, 1, n_push)
    assert need <= lib.at_encodec_workspace_bytes(h, 1, n_push + 640) + state
    x = _wav(1, total, seed=300).cuda()
    st = enc.new_stream(1)
    st.keep_embeddings = True
    codes, embs = [], []
    for i in range(pushes):
        codes.append(st.push(x[:, i * n_push:(i + 1) * n_push]).clone())
        embs.append(st.last_embeddings.clone())
        assert lib.at_encodec_stream_workspace_bytes(h, 1, n_push) == need, "the workspace of a push must not depend on what was pushed before"
    assert st.flush().shape[-1] == 0
    cs, es = torch.cat(codes, -1), torch.cat(embs, 1)
    assert cs.shape == (1, 8, 22500) and st.frames_emitted == 22500
    enc._ws = None                                # the stream's workspace: that of one 10 s window
    c1, e1 = _one_shot(enc, x)
    diff = (es - e1).abs().max().item()
    print(f"300 s in 10 s pushes: workspace {need / 2**20:.1f} MiB per push vs {lib.at_encodec_workspace_bytes(h, 1, total) / 2**20:.1f} MiB one-shot; "
          f"max |stream - one-shot| embedding difference {diff:.3e}")
    assert torch.equal(cs, c1) and torch.equal(es, e1)


# ---- 8. facade ------------------------------------------------------------------------------------------------------------------------
def test_facade_stream_equals_whole_file_and_default_did_not_move(tmp_path, enc_weights, cuda_device):
    from scipy.io import wavfile
    from audiotoken_amd import AudioToken, Tokenizers
    sr = 24000
    x = W.synth_waveform(1, 25 * sr, sr, seed=25)[0]
    path = tmp_path / "clip.wav"
    wavfile.write(str(path), sr, x)               # float32 WAV
    tok = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=8, weights=enc_weights)
    whole = tok.encode(path)
    streamed = tok.encode(path, chunk_size=10, stream=True)
    assert streamed.shape == (1, 8, 1875) and streamed.dtype == torch.int16
    assert torch.equal(streamed, whole)
    codes_ref, margins = R.acoustic_encode(enc_weights, torch.from_numpy(x)[None], 8, return_margins=True)
    P.assert_rvq_equal_or_explained(streamed, codes_ref, margins, P.RVQ_TIE, "encode(path, chunk_size=10, stream=True)")
    # the default chunked route: every chunk a clip of its own, batch dim dropped — as on the parent commit
    chunked = tok.encode(path, chunk_size=10)
    pieces = [tok.encoder(torch.from_numpy(x[i:i + 10 * sr])[None].cuda(), None).cpu()[0] for i in range(0, len(x), 10 * sr)]
    assert chunked.shape == (8, 1875) and torch.equal(chunked, torch.cat(pieces, dim=-1))
    for i in range(0, len(x), 10 * sr):
        ref, m = R.acoustic_encode(enc_weights, torch.from_numpy(x[i:i + 10 * sr])[None], 8, return_margins=True)
        P.assert_rvq_equal_or_explained(chunked[None, :, i // 320:i // 320 + ref.shape[-1]], ref, m, P.RVQ_TIE, f"default chunked route, chunk at {i}")
    assert not torch.equal(chunked, whole[0]), "per-chunk encoding starts every chunk from a fresh LSTM: its tokens are not the file's"
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.semantic_m, device="cuda:0").stream()
