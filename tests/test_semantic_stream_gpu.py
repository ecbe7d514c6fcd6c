"""GPU: the semantic-to-audio stream against the offline calls it is built from. The coarse ids, the finish reason, the window schedule and
the ``[8, T]`` fine codes of a stream are those of ``to_acoustic(long_form=True)`` and ``to_fine`` on the whole source with the same draws, under every
push schedule, with no tolerance: both sides run the same kernels on the same shapes at one row. The audio is that of a decode stream pushed the same
pieces. The offline calls are held to the float64 twins by their own tests."""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd import weights as W
from audiotoken_amd.configs import Wav2VecBertDecoderConfig
from audiotoken_amd.fine_decoder import fine_windows
from audiotoken_amd.fine_decoder import seeded_uniforms as fine_draws
from audiotoken_amd.semantic_decoder import seeded_uniforms
from audiotoken_amd.semantic_stream import SemanticAudioStream, stream_schedule

from tests import fine_cases
from tests import semantic_stream_cases as SC

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
S, H, WF = 8, 4, 128          # stage 1's window and hop, the fine model's block
# (N, max_new_tokens, window, hop). With finish == "max_new_tokens" the stream has 12 k + 12 + max_new ids after k non-final windows at (8, 4).
CASES = {
    "single": (5, 40, S, H),          # N <= S: one GPT window
    "short": (13, 20, S, H),          # 3 GPT windows, T < W
    "exact_a": (88, 4, S, H),         # 256 ids -> T = 128 = W: the last fine window is an eagerly run one
    "exact_b": (84, 16, S, H),        # 256 ids again, by another route
    "mid": (130, 7, S, H),            # W < T < 2 W, the last window at rel > 0
    "long": (176, 10, S, H),          # T > 2 W: at least 3 fine windows, the last reads emitted frames
    "wide": (41, 12, 16, 8),          # the other stage-1 geometry
}
SCHEDULES = ("all", "ones", "random", "at_window", "past_window")


@pytest.fixture(scope="module")
def sem():
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    return AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))


def source(N):
    return (np.arange(N) * 7 + N) % 1000


_offline = {}


def offline(sem, name, **trunc):
    """The offline calls of a case, computed once: (tokens, stage 1's draws, the AcousticGeneration, the fine draws, the [8, T] codes)."""
    key = (name, tuple(sorted(trunc.items())))
    if key not in _offline:
        N, max_new, s, h = CASES[name]
        tokens = source(N)
        u = seeded_uniforms(100 + N, 1, 3 * (N + s) + max_new + 64)
        coarse = sem.to_acoustic(tokens, long_form=True, window=s, hop=h, max_new_tokens=max_new, uniforms=u, **trunc)
        T = coarse.codes[0].shape[1]
        fu = fine_draws(200 + N, 1, len(fine_windows(T, WF)), WF)
        fine = sem.to_fine(coarse.codes, uniforms=fu)
        _offline[key] = (tokens, u, coarse, fu, fine.codes[0])
    return _offline[key]


def new_stream(sem, name, u, fu, **kw):
    N, max_new, s, h = CASES[name]
    return sem.audio_stream(window=s, hop=h, max_new_tokens=max_new, uniforms=None if u is None else u[0], fine_uniforms=None if fu is None else fu[0],
                            keep_codes=True, **kw)


def run_stream(st, tokens, pushes):
    """Push ``tokens`` in pieces of ``pushes`` ids and flush: the audio pieces of every call."""
    pieces, at = [], 0
    for n in pushes:
        pieces.append(st.push(tokens[at:at + n]))
        at += n
    pieces.append(st.flush())
    return pieces


def test_the_cases_cover_every_schedule(sem):
    """Asserted, so that the cases cannot silently degenerate: among the produced T one below W, one with (T - W) % H == 0, one past 2 W whose last
    window has rel > 0, and a source of at most S ids."""
    Ts = {name: offline(sem, name)[2].codes[0].shape[1] for name in CASES}
    print("frames per case:", Ts, {name: offline(sem, name)[2].finish[0] for name in CASES})
    Hf = WF // 2
    assert any(T < WF for T in Ts.values())
    assert any(T >= WF and (T - WF) % Hf == 0 for T in Ts.values())
    assert any(T > 2 * WF and (T - WF) % Hf != 0 for T in Ts.values())
    assert any(WF < T < 2 * WF and (T - WF) % Hf != 0 for T in Ts.values())
    assert CASES["single"][0] <= S and len(offline(sem, "single")[2].windows[0]) == 1
    assert len(offline(sem, "wide")[2].windows[0]) >= 3
    assert all(T >= 7 for T in Ts.values()), "every case can be decoded (the acoustic decoder needs 7 frames)"


@pytest.mark.parametrize("name", list(CASES))
def test_a_stream_equals_the_offline_calls_under_every_push_schedule(sem, name):
    tokens, u, coarse, fu, codes = offline(sem, name)
    N, max_new, s, h = CASES[name]
    T = codes.shape[1]
    st = new_stream(sem, name, u, fu)
    splits = SC.splittings(N, s, h)
    for schedule in SCHEDULES:
        st.reset()
        pieces = run_stream(st, tokens, splits[schedule])
        assert torch.equal(st.coarse_ids, coarse.ids[0]), (name, schedule)
        assert st.finish == coarse.finish[0] and st.windows == coarse.windows[0], (name, schedule)
        assert st.fine_windows_run == fine_windows(T, WF), (name, schedule)
        assert torch.equal(st.fine_codes, codes), (name, schedule)
        assert sum(p.shape[-1] for p in pieces) == 320 * T and st.frames_out == T and st.ids_in == N
        events = stream_schedule(splits[schedule], s, h, 3, 1024, WF, final_budget_result=coarse.windows[0][-1][3], max_new_tokens=max_new)
        emitted = [0 if e["emit"] is None else e["emit"][1] - e["emit"][0] for e in events]
        assert [p.shape[-1] // 320 for p in pieces] == emitted, "audio leaves the call in which its frames turn final"


def test_a_single_window_source_equals_the_short_form(sem):
    tokens, u, coarse, fu, codes = offline(sem, "single")
    N, max_new, s, h = CASES["single"]
    short = sem.to_acoustic(tokens, max_new_tokens=max_new, uniforms=u[:, :max_new], constrain=True)
    st = new_stream(sem, "single", u, fu)
    run_stream(st, tokens, [2, 3])
    assert torch.equal(st.coarse_ids, short.ids[0]) and st.finish == short.finish[0]


@pytest.mark.parametrize("name", ["short", "long"])
def test_the_audio_is_that_of_a_decode_stream_pushed_the_same_pieces(sem, name):
    tokens, u, coarse, fu, codes = offline(sem, name)
    N, max_new, s, h = CASES[name]
    T = codes.shape[1]
    st = new_stream(sem, name, u, fu)
    pieces = run_stream(st, tokens, SC.splittings(N, s, h)["random"])
    frames = [p.shape[-1] // 320 for p in pieces]
    assert all(p.dtype == torch.float32 and p.dim() == 2 and p.shape[0] == 1 and p.shape[1] % 320 == 0 for p in pieces) and sum(frames) == T
    acoustic = sem._fine_audio()
    ref = acoustic.decode_stream()
    at, first = 0, True
    for p, n in zip(pieces, frames):
        if n == 0:
            continue
        cut = codes[:, at:at + n].unsqueeze(0).to(DEV)
        want = ref.push(cut).cpu()
        assert torch.equal(p, want), (name, at, n)
        if first:   # the existing property of a stream's first push
            assert torch.equal(p, acoustic.decode(codes[:, :n].unsqueeze(0)).cpu()), "the first piece is a one-shot decode of its frames"
            first = False
        at += n
    assert at == T and ref.flush().shape[-1] == 0


def test_reset_and_interleaved_streams_leak_nothing(sem):
    tl, ul, cl, ful, codes_l = offline(sem, "long")
    ts, us, cs, fus, codes_s = offline(sem, "short")
    # a short source after a long one in the same object, with the short case's draws: explicit draws belong to the object, so use the seed form
    a = sem.audio_stream(window=S, hop=H, max_new_tokens=CASES["short"][1], seed=5, keep_codes=True)
    run_stream(a, tl, [50, 126])
    a.reset()
    after = run_stream(a, ts, [6, 7])
    ids_after, codes_after = a.coarse_ids, a.fine_codes
    b = sem.audio_stream(window=S, hop=H, max_new_tokens=CASES["short"][1], seed=5, keep_codes=True)
    fresh = run_stream(b, ts, [6, 7])
    assert torch.equal(ids_after, b.coarse_ids) and torch.equal(codes_after, b.fine_codes)
    assert all(torch.equal(x, y) for x, y in zip(after, fresh))
    # from seed=, the stream's lazy draws are the prefixes of what the offline call draws for one source
    _, coarse, fine = sem.to_audio(ts, long_form=True, window=S, hop=H, max_new_tokens=CASES["short"][1], seed=5)
    assert torch.equal(b.coarse_ids, coarse.ids[0]) and torch.equal(b.fine_codes, fine.codes[0])
    # two objects interleaved push by push each equal their solo run
    x, y = new_stream(sem, "long", ul, ful), new_stream(sem, "mid", *offline(sem, "mid")[1::2])
    tm = offline(sem, "mid")[0]
    px, py = SC.splittings(len(tl), S, H)["random"], SC.splittings(len(tm), S, H)["random"]
    ax = ay = 0
    for i in range(max(len(px), len(py))):
        if i < len(px):
            x.push(tl[ax:ax + px[i]]); ax += px[i]
        if i < len(py):
            y.push(tm[ay:ay + py[i]]); ay += py[i]
    x.flush(); y.flush()
    assert torch.equal(x.fine_codes, codes_l) and torch.equal(x.coarse_ids, cl.ids[0])
    assert torch.equal(y.fine_codes, offline(sem, "mid")[4]) and torch.equal(y.coarse_ids, offline(sem, "mid")[2].ids[0])


def test_the_states_do_not_grow_with_the_source(sem):
    gpt, fine = sem._gpt(), sem._fine()
    want = (int(gpt._fn("stream_state_bytes")(gpt.handle, S, H, 3)), int(fine._fn("stream_state_bytes")(fine.handle)))
    short, long_ = new_stream(sem, "short", *offline(sem, "short")[1::2]), new_stream(sem, "long", *offline(sem, "long")[1::2])
    assert short.state_bytes == long_.state_bytes == want and min(want) > 0
    held = long_._gpt_state.data_ptr(), long_._fine_state.data_ptr()
    run_stream(long_, offline(sem, "long")[0], [176])
    assert long_.state_bytes == want and held == (long_._gpt_state.data_ptr(), long_._fine_state.data_ptr()), "a source past 2 W frames ran in the same state"
    assert torch.equal(long_.fine_codes, offline(sem, "long")[4])
    assert want[1] == int(fine._fn("state_bytes")(fine.handle, 1, 2 * WF)), "the fine state is one row of 2 W cells"


def test_truncation_is_the_offline_calls(sem):
    tokens, u, coarse, fu, codes = offline(sem, "short", top_p=0.9, min_p=0.05)
    plain = offline(sem, "short")[2]
    assert plain.ids[0].tolist() != coarse.ids[0].tolist(), "the truncation changes what this case draws"
    st = new_stream(sem, "short", u, fu, top_p=0.9, min_p=0.05)
    run_stream(st, tokens, [4, 5, 4])
    assert torch.equal(st.coarse_ids, coarse.ids[0]) and st.finish == coarse.finish[0] and torch.equal(st.fine_codes, codes)


def test_the_hand_over_reports_an_id_outside_its_code_book(sem):
    lib = _cabi.load()
    off, cb = 2000, 1024
    ids = torch.tensor([off + 5, off + cb + 6, off + 7, off + 8, off - 1, off + cb + 9, off + 10, off + 2 * cb, off + 1023, off + cb + 1023],
                       dtype=torch.int32, device=DEV)   # frame 1: code book 1 holds a code book 0 id; frame 2: below; frame 3: past code book 1
    work = torch.full((7, 8), -7, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.cuda.device(DEV):
        _cabi.check(lib.at_op_fine_handover(ids.data_ptr(), 5, 2, off, cb, work.data_ptr(), _cabi.current_stream_handle(torch.device(DEV)), status.data_ptr()),
                    "at_op_fine_handover")
    got = work.cpu()
    assert int(status.item()) == 4
    assert got[0].tolist() == [5, 6] + [1024] * 6 and got[4].tolist() == [1023, 1023] + [1024] * 6
    assert bool((got[1:4] == -7).all()), "a frame with an id outside its code book is not written"
    assert bool((got[5:] == 1024).all()), "the padding cells hold 1024 in all 8 channels"
    status.zero_()
    with torch.cuda.device(DEV):
        _cabi.check(lib.at_op_fine_handover(ids.data_ptr(), 1, 0, off, cb, work.data_ptr(), _cabi.current_stream_handle(torch.device(DEV)), status.data_ptr()),
                    "at_op_fine_handover")
    assert int(status.item()) == 0


def test_refusals_raise_before_any_launch_and_leave_the_object_usable(sem):
    tokens, u, coarse, fu, codes = offline(sem, "short")
    with pytest.raises(ValueError, match="voice= is not built"):
        sem.audio_stream(voice=object())
    with pytest.raises(ValueError, match="has no semantic ids"):
        AudioToken(Tokenizers.acoustic, device=DEV).audio_stream()
    with pytest.raises(ValueError, match="top_p"):
        sem.audio_stream(top_p=1.5)
    with pytest.raises(ValueError, match="long form"):
        sem.audio_stream(window=8, hop=10)
    st = new_stream(sem, "short", u, fu)
    with pytest.raises(RuntimeError, match="nothing pushed"):
        st.flush()
    with pytest.raises(ValueError, match="semantic ids must lie"):
        st.push([1, 2, 10 ** 6])
    assert st.push([]).shape == (1, 0) and st.ids_in == 0, "an empty push is allowed"
    run_stream(st, tokens, [13])
    assert torch.equal(st.fine_codes, codes), "the refusals above left the object usable"
    with pytest.raises(RuntimeError, match="push after flush"):
        st.push(tokens[:2])
    with pytest.raises(RuntimeError, match="twice"):
        st.flush()
    st.reset()
    run_stream(st, tokens, [7, 6])
    assert torch.equal(st.fine_codes, codes)
    # explicit draws that run out: refused before the window that would need them, and the pushes before it stand
    few = sem.audio_stream(window=S, hop=H, max_new_tokens=20, uniforms=u[0, :30], fine_uniforms=fu[0], keep_codes=True)
    few.push(tokens[:9])                      # window 0: positions 0 to 23
    with pytest.raises(ValueError, match="uniforms: the stream needs entry"):
        few.push(tokens[9:13])                # window 1 needs positions 24 to 35
    assert few.ids_in == 9 and torch.equal(few.coarse_ids, coarse.ids[0][:24])
    # the library's own record: a push after the final call is refused by the C entry too, before the device is touched
    gpt = sem._gpt()
    pos = (C.c_int64 * 2)(13, 1)
    rc = gpt._fn("stream_push")(gpt.handle, st._gpt_state.data_ptr(), st._gpt_state.numel(), pos, st._len.data_ptr(), 1, 0, S, H, 3, 0, 1000, 1, 2, 1024, 3, 20, 0.8,
                                100, st._len.data_ptr(), 0, 0, st._len.data_ptr(), 0, st._len.data_ptr(), st._fin.data_ptr(), None, None, None)
    assert rc != 0 and "after the final call" in _cabi.last_error()


def test_a_stream_without_a_whole_frame_raises_what_to_audio_raises(sem):
    tokens = source(5)
    u = np.zeros((1, 64), dtype=np.float32)
    coarse = sem.to_acoustic(tokens, long_form=True, window=S, hop=H, max_new_tokens=1, uniforms=u)
    assert coarse.codes[0] is None or coarse.codes[0].shape[1] == 0
    with pytest.raises(ValueError, match="produced no whole frame"):
        sem.to_audio(tokens, long_form=True, window=S, hop=H, max_new_tokens=1, uniforms=u)
    st = sem.audio_stream(window=S, hop=H, max_new_tokens=1, uniforms=u[0])
    st.push(tokens)
    with pytest.raises(ValueError, match="produced no whole frame"):
        st.flush()
