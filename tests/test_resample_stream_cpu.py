"""CPU: the host side of the streaming resampler (audiotoken_amd/resample_stream.py).

* the planner: for every rate and a schedule of pushes of 1 sample, width - 1, o, o + 1, 4096 and a random remainder (tests/resample_stream_cases.py), the
  emitted ranges tile [0, ceil(n L / o)), every tap of every emitted sample is in the push's window or outside the signal (and that only on the final
  push), the carried tail stays below 2 width + o samples, and a float64 evaluation of the chunked plan (float32 table) EQUALS the evaluation of the whole;
* ``at_resample_rows_check`` through ctypes: every rejection it documents, one accepted row per rate;
* ``resample=`` argument errors are raised before a model is loaded;
* ``AcousticStream(sample_rate=...)`` and ``AcousticStreamPool.open(sample_rate=...)`` on stubs: the resampled samples reach the library stub in order,
  none lost across a push that holds everything back.
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd import resample_stream as RS
from audiotoken_amd.streaming import FIRST_PUSH_FRAMES, HOP, AcousticStream, AcousticStreamPool
from tests import resample_stream_cases as X

MODEL = X.MODEL_RATE


# ---- the planner ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flush_empty", (False, True), ids=("last_push_final", "empty_flush"))
@pytest.mark.parametrize("rate", X.RATES)
def test_plan_tiles_the_output_and_every_tap_is_in_its_window(rate, flush_empty):
    L = X.signal_length(rate)
    o, n, width = RS.ratio(rate, MODEL)
    sizes = X.push_sizes(rate, L)
    assert sum(sizes) == L and {1, o, o + 1, 4096} <= set(sizes) and (width < 2 or width - 1 in sizes)
    nxt = 0
    for start, plan, tail_before in X.plans(rate, sizes, flush_empty):
        assert tail_before <= 2 * width + o, "the carried tail exceeds 2 width + o samples"
        assert plan.keep < 2 * width + o or (o == n and plan.keep == 0)
        assert plan.out_start == nxt and plan.out_len >= 0, "gap or overlap between the emitted ranges"
        nxt = plan.out_start + plan.out_len
        assert plan.src_base + tail_before == start, "the window is the tail followed by the new samples"
        if plan.out_len == 0:
            continue
        first_tap = (plan.out_start // n) * o - width                  # tap 0 of the first output's frame
        last_tap = ((nxt - 1) // n) * o + width + o - 1                # tap kw - 1 of the last output's frame
        w_lo, w_hi = plan.src_base, plan.src_base + plan.src_len
        if plan.final:       # a tap may lie outside the signal now, and only now; inside the signal it is in the window
            assert plan.src_total == L
            assert max(first_tap, 0) >= w_lo and min(last_tap, L - 1) < w_hi
        else:
            assert first_tap >= w_lo and last_tap < w_hi, "a tap outside the window before the end of the signal is known"
    assert nxt == -(-n * L // o) == RS.ceil_div(n * L, o)


@pytest.mark.parametrize("rate", X.RATES)
def test_single_sample_pushes_tile_too(rate):
    """Every push one sample (a short signal: the plan is integers only): nothing is emitted before a frame is ready, everything by the end."""
    o, n, width = RS.ratio(rate, MODEL)
    L = 3 * (2 * width + o) + 5
    pos, nxt = RS.StreamPosition(o, n, width), 0
    for i in range(L):
        plan = RS.plan_push(pos, 1, i == L - 1)
        assert plan.out_start == nxt and pos.tail_len <= 2 * width + o
        if not plan.final and plan.out_len:
            assert ((nxt + plan.out_len - 1) // n) * o + width + o <= i + 1, "a frame emitted before its last tap has arrived"
        nxt += plan.out_len
        RS.commit(pos, plan)
    assert nxt == RS.ceil_div(n * L, o)


@pytest.mark.parametrize("rate", X.RATES)
def test_chunked_evaluation_equals_the_whole_signal_exactly(rate):
    x = X.signal(rate).astype(np.float64)
    L = len(x)
    o, n, width = RS.ratio(rate, MODEL)
    whole = RS.evaluate_plan(x, RS.PushPlan(0, RS.ceil_div(n * L, o), 0, L, L, True, 0, 0), rate, MODEL)
    padded = np.concatenate([np.zeros(width), x])       # the stream's stored zeros at -width .. -1, then the signal
    parts = []
    for start, plan, tail_before in X.plans(rate, X.push_sizes(rate, L), True):
        window = padded[plan.src_base + width:plan.src_base + width + plan.src_len]
        parts.append(RS.evaluate_plan(window, plan, rate, MODEL))
    got = np.concatenate(parts)
    assert got.shape == whole.shape and np.array_equal(got, whole), f"{int((got != whole).sum())} samples differ, max {np.abs(got - whole).max():.3e}"
    if rate != MODEL:       # and the rule is the project's resampler: audio_io.resample sums the same products in another order
        from audiotoken_amd.audio_io import resample
        ref = resample(torch.from_numpy(X.signal(rate).copy())[None], rate, MODEL)[0].numpy()
        assert np.abs(whole - ref).max() < 1e-5


def test_file_ticks_tile_the_file():
    for rate in X.RATES:
        L = X.signal_length(rate)
        o, n, width = RS.ratio(rate, MODEL)
        nxt = 0
        for c in range(RS.ceil_div(L, rate)):
            plan = RS.file_tick_plan(L, o, n, rate, c)
            assert plan.out_start == nxt and plan.out_len == min(MODEL, RS.ceil_div(n * L, o) - nxt) and plan.final and plan.src_len == L
            nxt += plan.out_len
        assert nxt == RS.ceil_div(n * L, o)


# ---- the checker ------------------------------------------------------------------------------------------------------------------------------------
FAKE = 0x10000     # an address the checker must never read


def _row(plan, rate, **over):
    o, n, width = RS.ratio(rate, MODEL)
    fields = dict(zip([f[0] for f in _cabi.ResampleRow._fields_], plan.row(FAKE, FAKE if rate != MODEL else 0, _cabi.PCM_S16, 1.0 / 32768.0, o, n, width, 0)))
    fields.update(over)
    return _cabi.ResampleRow(**fields)


def _check(rows, nrows=None):
    arr = (_cabi.ResampleRow * max(len(rows), 1))(*rows)
    rc = _cabi.load().at_resample_rows_check(C.addressof(arr), len(rows) if nrows is None else nrows)
    return rc, _cabi.last_error()


def _first_push(rate, n_new=4096):
    return RS.plan_push(RS.StreamPosition(*RS.ratio(rate, MODEL)), n_new, False)


def _whole(rate, L=4096):
    o, n, width = RS.ratio(rate, MODEL)
    return RS.PushPlan(0, RS.ceil_div(n * L, o), 0, L, L, True, 0, 0)


@pytest.mark.parametrize("rate", X.RATES)
def test_checker_accepts_what_the_planner_plans(rate):
    rows = [_row(plan, rate) for _, plan, _ in X.plans(rate, X.push_sizes(rate, X.signal_length(rate)), True)] + [_row(_whole(rate), rate)]
    rc, err = _check(rows)
    assert rc == 0, err


def test_checker_rejections():
    lib = _cabi.load()
    rate = 44100
    good, whole = _first_push(rate), _whole(rate)
    assert _check([_row(good, rate)])[0] == 0 and _check([_row(whole, rate)])[0] == 0
    assert lib.at_resample_rows_check(None, 1) != 0 and "null descriptor list" in _cabi.last_error()
    for nrows in (0, -1):
        rc, err = _check([_row(good, rate)], nrows)
        assert rc != 0 and "nrows" in err
    cases = [
        (_row(good, rate, pcm=0), "null pcm"),
        (_row(good, rate, table=0), "null resampling table"),
        (_row(good, rate, out_len=-1), "negative out_len"),
        (_row(good, rate, fmt=4), "unknown sample format"),
        (_row(good, rate, fmt=-1), "unknown sample format"),
        (_row(good, rate, width=11), "do not belong together"),
        (_row(good, rate, o=294, n=160), "do not belong together"),
        (_row(good, rate, o=160, n=147), "do not belong together"),          # 48 kHz's ratio with 44.1 kHz's width
        (_row(good, rate, o=1, n=1, width=0), "do not belong together"),     # the native rate has no table
        (_row(good, rate, out_len=good.out_len + 80), "not final with a tap outside"),     # a frame that is not ready
        (_row(good, rate, src_base=0), "not final with a tap outside"),                    # no stored zeros in front
        (_row(good, rate, src_len=good.src_len - 147), "not final with a tap outside"),
        (_row(whole, rate, src_base=1, src_len=4095), "final row with a tap inside"),
        (_row(whole, rate, src_len=4095), "final row with a tap inside"),
        (_row(whole, rate, out_len=whole.out_len + 1), "past the end"),
        (_row(whole, rate, src_total=-1), "src_total"),
        (_row(good, rate, out_start=-80), "negative"),
        (_row(good, rate, dst_off=-1), "negative"),
    ]
    for row, text in cases:
        rc, err = _check([_row(good, rate), row])
        assert rc != 0 and text in err and "row 1" in err, (text, rc, err)
    # a tap outside the signal is fine on a final row: the signal's end, and its start when the window opens at sample 0
    assert _check([_row(whole, rate)])[0] == 0


# ---- argument errors: before a model is loaded ----------------------------------------------------------------------------------------------------------
def test_resample_argument_errors_come_before_the_model(tmp_path):
    at = AudioToken(Tokenizers.acoustic, device="cuda:0")
    path = Path(tmp_path / "x.wav")
    with pytest.raises(ValueError, match="resample"):
        at.encode(path, chunk_size=1, stream=True, resample="nope")
    with pytest.raises(ValueError, match="stream=True"):
        at.encode(path, chunk_size=1, resample="file")
    with pytest.raises(ValueError, match="resample"):
        at.encode_batch_files(batch_size=2, outdir=tmp_path / "out", chunk_size=1, audio_files=[path], stream=True, resample="nope")
    with pytest.raises(ValueError, match="stream=True"):
        at.encode_batch_files(batch_size=2, outdir=tmp_path / "out", chunk_size=1, audio_files=[path], resample="file")
    assert at.encoder is None, "the refusal must come before any model is loaded"
    sem = AudioToken(Tokenizers.semantic_m, device="cuda:0")
    with pytest.raises(ValueError, match="acoustic"):
        sem.encode(path, chunk_size=1, stream=True, resample="file")
    with pytest.raises(ValueError, match="acoustic"):
        sem.stream(sample_rate=44100)
    assert sem.encoder is None


# ---- the streams on stubs ---------------------------------------------------------------------------------------------------------------------------------
class _Stub:
    """push_fn stand-in: records what the library would be given."""

    def __init__(self, n_q):
        self.n_q, self.calls, self.seen = n_q, [], []

    def __call__(self, x, final, started=None):
        assert x.is_contiguous() and x.dtype == torch.float32
        self.calls.append((x.shape[1], final))
        self.seen.append(x.clone())
        return torch.zeros(x.shape[0], self.n_q, -(-x.shape[1] // HOP), dtype=torch.int16)


def _whole_resampled(x_pcm: torch.Tensor, rate: int) -> torch.Tensor:
    """What the stand-in resampler gives for the whole signal in one final push."""
    L = x_pcm.shape[-1]
    o, n, width = RS.ratio(rate, MODEL)
    plan = RS.PushPlan(0, RS.ceil_div(n * L, o), 0, L, L, True, 0, 0)
    return RS.HostResampler(MODEL).run([RS.Job(x_pcm, rate, plan)])[0]


@pytest.mark.parametrize("rate,kind", [(44100, "int16"), (8000, "float32"), (48000, "numpy_int16"), (24000, "int16")])
def test_stub_stream_gets_the_whole_signal_resampled_in_order(rate, kind):
    x = X.signal(rate)
    pcm = torch.from_numpy(np.round(x * 32767.0).astype(np.int16)) if "int16" in kind else torch.from_numpy(x.copy())
    B = 2
    both = torch.stack([pcm, pcm.flip(0)])
    stub = _Stub(4)
    st = AcousticStream(None, B, push_fn=stub, n_q=4, sample_rate=rate)
    # the first pushes are too short to release the first 7 frames: everything resampled so far must be held, not lost
    sizes = [5, 300] + X.push_sizes(rate, len(x) - 305)
    outs, pos = [], 0
    for i, s in enumerate(sizes):
        piece = both[:, pos:pos + s]
        outs.append(st.push(piece.numpy() if kind.startswith("numpy") else piece))
        if i < 2:
            assert outs[-1].shape[-1] == 0 and stub.calls == []
        pos += s
    outs.append(st.flush())
    want = torch.stack([_whole_resampled(both[b], rate) for b in range(B)])
    got = torch.cat(stub.seen, dim=1)
    assert got.shape == want.shape and torch.equal(got, want), "the library did not get the whole signal's resampled samples, in order"
    assert [f for _, f in stub.calls] == [False] * (len(stub.calls) - 1) + [True]
    assert all(n % HOP == 0 for n, f in stub.calls if not f) and stub.calls[0][0] >= FIRST_PUSH_FRAMES * HOP
    assert torch.cat(outs, dim=-1).shape[-1] == -(-want.shape[1] // HOP) == st.frames_emitted
    with pytest.raises(RuntimeError, match="after flush"):
        st.push(both[:, :10])
    st.reset()       # a new stream: the tail and the position start over
    st.push(both)
    st.flush()
    assert torch.equal(torch.cat(stub.seen, dim=1)[:, want.shape[1]:], want)


def test_stub_stream_refuses_other_formats():
    st = AcousticStream(None, 1, push_fn=_Stub(4), n_q=4, sample_rate=16000)
    with pytest.raises(TypeError, match="float32 or int16"):
        st.push(torch.zeros(1, 100, dtype=torch.float64))
    st.push(torch.zeros(1, 100, dtype=torch.int16))
    with pytest.raises(TypeError, match="first push"):
        st.push(torch.zeros(1, 100, dtype=torch.float32))


def test_stub_pool_mixes_rates_in_one_resample_call():
    stub = _Stub(4)
    rs = RS.HostResampler(MODEL)
    pool = AcousticStreamPool(None, 3, push_fn=stub, gather_fn=lambda slots: None, scatter_fn=lambda slots: None, n_q=4, resampler=rs)
    a, b, c = pool.open(sample_rate=48000), pool.open(sample_rate=16000), pool.open()
    xa = torch.from_numpy(np.round(X.signal(48000) * 32767.0).astype(np.int16))
    xb = torch.from_numpy(X.signal(16000).copy())
    xc = torch.from_numpy(X.signal(24000).copy())
    got = {a: [], b: [], c: []}
    run = pool._run

    def spy(ids, xs, started, final, out):      # what every stream hands the library, whichever streams share the push
        for sid, x in zip(ids, xs):
            got[sid].append(x.clone())
        return run(ids, xs, started, final, out)
    pool._run = spy
    steps = 4
    for i in range(steps):
        pool.push({sid: x[i * len(x) // steps:(i + 1) * len(x) // steps] for sid, x in ((a, xa), (b, xb), (c, xc))})
        assert rs.launches == i + 1, "the streams of one call share one resample call"
    pool.flush([a, b, c])
    assert rs.launches == steps + 1 and pool.live == []
    assert torch.equal(torch.cat(got[a]), _whole_resampled(xa, 48000))
    assert torch.equal(torch.cat(got[b]), _whole_resampled(xb, 16000))
    assert torch.equal(torch.cat(got[c]), xc)
    assert all(f or n % HOP == 0 for n, f in stub.calls)
