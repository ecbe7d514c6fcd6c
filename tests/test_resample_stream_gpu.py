"""GPU: the streaming resampler (csrc/stream_resample.hip, audiotoken_amd/resample_stream.py).

The yardstick is the feeder's kernel, ``at_segments_from_pcm``, run ONCE on the whole signal as one chunk (``seg_len`` = the resampled length): it computes
the rule at chunk-local positions, which for one chunk are the signal's. What is asserted:
* kernel, bit-exact: rows cut at pushes of 1 sample, width - 1, o, o + 1, 4096 and a random remainder, all in one launch, are ``torch.equal`` to it, for
  every rate and for s16, s32, f32 and u8 samples;
* kernel, accuracy: <= 1e-6 from oracle/resample_ref.sinc_interp_hann (float64 per output sample), the bar tests/test_feeder_gpu.py holds the feeder to;
* one launch that mixes rates, formats and lengths writes each row's ``out_len`` floats and nothing else (sentinel);
* 64-bit positions: a row shifted by 2^33 frames gives the unshifted row's outputs (away from the signal's first ``width`` samples);
* ``encode(path, chunk_size=1, stream=True, resample="file")`` == ``encode`` of the whole-signal device-resampled waveform (per-chunk resampling cannot:
  its seams are 0.05 at 44.1 kHz and 0.13 at 8 kHz);
* live streams at their own rate (int16, ragged pushes; a pool with a 48 kHz and a 16 kHz stream) give the tokens of ``stream()`` fed that waveform;
* ``encode_batch_files(stream=True, resample="file")`` over WAV s16 / f32 / u8, FLAC and a tar: every token file is that of the file's whole-signal waveform.

Fixture files: 16-bit WAV and FLAC by the project's writers (audio_io.save_audio); float32 and 8-bit WAV, which they do not write, by scipy.
"""
import ctypes as C
import tarfile
from pathlib import Path

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import audio_io as A
from audiotoken_amd import resample_stream as RS
from audiotoken_amd import weights as W
from oracle import resample_ref as RR
from tests import resample_stream_cases as X

pytestmark = pytest.mark.gpu
MODEL, HOP = X.MODEL_RATE, 320
FORMATS = ["s16", "s32", "f32", "u8"]
DEV = "cuda:0"


@pytest.fixture(scope="module")
def resampler(cuda_device):
    return RS.DeviceResampler(DEV, MODEL)


_WHOLE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_device_memory():
    """The module's shared references go when it is done, and with them the allocator's cached blocks: the modules after it start as they did before."""
    yield
    _WHOLE.clear()
    _TOKENS.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def whole_signal(resampler, rate, fmt):
    """``(pcm on the device, AT_PCM code, scale, at_segments_from_pcm of the whole signal as one chunk [Lr])`` — computed once per (rate, format)."""
    key = (rate, fmt)
    if key not in _WHOLE:
        arr, code, scale = X.as_format(X.signal(rate), fmt)
        pcm = torch.from_numpy(arr).to(DEV)
        L = len(arr)
        tptr, o, n, width = resampler.table(rate)
        Lr = RS.ceil_div(n * L, o)
        desc = _cabi.SegmentDesc(pcm.data_ptr(), tptr, 0, L, 0, Lr, code, scale, o, n, width, Lr)
        d_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
        out = torch.full((Lr,), float("nan"), dtype=torch.float32, device=DEV)
        _cabi.check(resampler.lib.at_segments_from_pcm(d_dev.data_ptr(), 1, Lr, 0.0, out.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                    "at_segments_from_pcm")
        torch.cuda.synchronize()
        assert not torch.isnan(out).any()
        _WHOLE[key] = (pcm, code, scale, out)
    return _WHOLE[key]


def pushed_jobs(pcm, code, scale, rate, flush_empty=True):
    """The signal as a stream's pushes: one Job per push, its window a slice of (stored zeros + signal) on the device."""
    o, n, width = RS.ratio(rate, MODEL)
    zero = torch.full((width,), 128 if pcm.dtype == torch.uint8 else 0, dtype=pcm.dtype, device=pcm.device)
    padded = torch.cat([zero, pcm])
    jobs = []
    for _, plan, _ in X.plans(rate, X.push_sizes(rate, pcm.numel()), flush_empty):
        a = plan.src_base + width
        jobs.append(RS.Job(padded[a:a + plan.src_len], rate, plan, code, scale))
    return jobs


@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("rate", X.RATES)
def test_rows_cut_at_pushes_equal_the_whole_signal_kernel(resampler, rate, fmt):
    pcm, code, scale, want = whole_signal(resampler, rate, fmt)
    jobs = pushed_jobs(pcm, code, scale, rate)
    before = resampler.launches
    got = torch.cat(resampler.run(jobs))
    assert resampler.launches == before + 1 and len(jobs) > 10
    bad = int((got != want).sum()) if got.shape == want.shape else -1
    print(f"{rate} Hz {fmt}: {len(jobs)} rows, {got.numel()} outputs, {bad} differ")
    assert got.shape == want.shape and torch.equal(got, want), f"{bad} of {want.numel()} samples differ from at_segments_from_pcm on the whole signal"


@pytest.mark.parametrize("rate", [r for r in X.RATES if r != MODEL])
def test_accuracy_against_the_float64_oracle(resampler, rate):
    pcm, code, scale, _ = whole_signal(resampler, rate, "s16")
    got = torch.cat(resampler.run(pushed_jobs(pcm, code, scale, rate, flush_empty=False))).cpu().numpy()
    x = pcm.cpu().numpy().astype(np.float32) * np.float32(scale)
    ref = RR.sinc_interp_hann(x, rate, MODEL)
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{rate} Hz: max |device - oracle| = {err:.3e}")
    assert got.shape == ref.shape and err <= 1e-6


def test_one_launch_mixes_rates_formats_and_lengths_and_writes_only_its_rows(resampler):
    """Rows of four rates in four formats, of lengths from 0 to several blocks, at odd destinations of a sentinel-filled buffer, in one launch."""
    lib = resampler.lib
    picks = [(44100, "s16"), (8000, "u8"), (24000, "f32"), (48000, "s32"), (22050, "f32"), (24000, "s16")]
    rows, want, keep = [], [], []
    off = 3                                    # an odd start: the first row is not 16-byte aligned
    for rate, fmt in picks:
        pcm, code, scale, whole = whole_signal(resampler, rate, fmt)
        tptr, o, n, width = resampler.table(rate)
        jobs = pushed_jobs(pcm, code, scale, rate)
        for j in jobs[3:9]:                    # a run of consecutive pushes of this signal, among them one that emits nothing
            # (a push of nothing at the native rate has an empty window, whose tensor has no address: any valid one serves, it is never read)
            rows.append(_cabi.ResampleRow(*j.plan.row(j.pcm.data_ptr() or pcm.data_ptr(), tptr, code, scale, o, n, width, off)))
            want.append((off, whole[j.plan.out_start:j.plan.out_start + j.plan.out_len]))
            keep.append(j.pcm)
            off += j.plan.out_len + (len(rows) % 3)      # gaps of 0, 1 or 2 floats between rows
    assert any(len(w) == 0 for _, w in want) and any(len(w) > 2048 for _, w in want)
    arr = (_cabi.ResampleRow * len(rows))(*rows)
    _cabi.check(lib.at_resample_rows_check(C.addressof(arr), len(rows)), "at_resample_rows_check")
    d_rows = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(DEV)
    SENT = -123.0
    out = torch.full((off + 64,), SENT, dtype=torch.float32, device=DEV)
    _cabi.check(lib.at_resample_rows(d_rows.data_ptr(), len(rows), out.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "at_resample_rows")
    torch.cuda.synchronize()
    touched = torch.zeros_like(out, dtype=torch.bool)
    for o_, w in want:
        assert torch.equal(out[o_:o_ + len(w)], w)
        touched[o_:o_ + len(w)] = True
    assert bool((out[~touched] == SENT).all()), "a float outside every row's out_len was written"
    assert int((~touched).sum()) >= 64


@pytest.mark.parametrize("rate,fmt", [(44100, "s16"), (8000, "f32"), (24000, "s16")])
def test_positions_beyond_32_bits(resampler, rate, fmt):
    """src_base and out_start shifted by 2^33 frames (2^33 o source samples, 2^33 n outputs): the same window, the same outputs — from the first frame whose
    taps do not reach before the window (the unshifted row has zeros there, the shifted one would have earlier samples of its stream)."""
    pcm, code, scale, whole = whole_signal(resampler, rate, fmt)
    o, n, width = RS.ratio(rate, MODEL)
    L, Lr = pcm.numel(), whole.numel()
    j1 = n * RS.ceil_div(width, o)
    shift = 1 << 33
    plain = RS.PushPlan(j1, Lr - j1, 0, L, L, True, 0, 0)
    moved = RS.PushPlan(shift * n + j1, Lr - j1, shift * o, L, shift * o + L, True, 0, 0)
    a, b = resampler.run([RS.Job(pcm, rate, plain, code, scale), RS.Job(pcm, rate, moved, code, scale)])
    assert torch.equal(a, whole[j1:]) and torch.equal(b, a), f"{int((b != a).sum())} outputs differ 2^33 frames into the stream"


# ---- through the encoder ------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tok(cuda_device):
    from audiotoken_amd import AudioToken, Tokenizers
    return AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8, weights=W.synth_encodec_weights(seed=0, with_decoder=False))


def s16(rate):
    return X.as_format(X.signal(rate), "s16")[0]


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    """The directory of the batch test; the 44.1 kHz and 8 kHz files also serve ``encode``."""
    from scipy.io import wavfile
    src = tmp_path_factory.mktemp("rates")
    A.save_audio(s16(44100).astype(np.float32) / 32768.0, src / "a_44k_s16.wav", 44100)
    wavfile.write(str(src / "b_48k_f32.wav"), 48000, X.signal(48000)[:48000].copy())        # exactly 1.0 s
    A.save_audio(s16(24000).astype(np.float32) / 32768.0, src / "c_24k_s16.wav", 24000)
    A.save_audio(s16(22050).astype(np.float32) / 32768.0, src / "d_22k.flac", 22050)
    wavfile.write(str(src / "e_8k_u8.wav"), 8000, X.as_format(X.signal(8000), "u8")[0])
    with tarfile.open(src / "f_members.tar", "w") as tar:
        tar.add(src / "a_44k_s16.wav", arcname="in_tar_44k.wav")
        tar.add(src / "d_22k.flac", arcname="in_tar_22k.flac")
    return src


_TOKENS = {}


def whole_file_tokens(tok, resampler, path):
    """``encode`` of the file's whole-signal waveform: the file decoded to its storage format, resampled by at_segments_from_pcm as one chunk."""
    key = str(path)
    if key not in _TOKENS:
        from audiotoken_amd.feeder import _FMT
        raw = A.decode_raw(str(path))
        assert raw.pcm.shape[0] == 1
        pcm = torch.from_numpy(raw.pcm[0].copy()).to(DEV)
        L = pcm.numel()
        tptr, o, n, width = resampler.table(raw.sample_rate)
        Lr = RS.ceil_div(n * L, o)
        desc = _cabi.SegmentDesc(pcm.data_ptr(), tptr, 0, L, 0, Lr, _FMT[raw.pcm.dtype], float(raw.scale), o, n, width, Lr)
        d_dev = torch.from_numpy(np.frombuffer(desc, dtype=np.uint8).copy()).to(DEV)
        wav = torch.empty((1, Lr), dtype=torch.float32, device=DEV)
        _cabi.check(resampler.lib.at_segments_from_pcm(d_dev.data_ptr(), 1, Lr, 0.0, wav.data_ptr(), None, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                    "at_segments_from_pcm")
        torch.cuda.synchronize()
        _TOKENS[key] = (wav, tok.encode(wav.cpu()))
    return _TOKENS[key]


def test_fixture_files_hold_the_signals(corpus):
    raw = A.decode_raw(str(corpus / "a_44k_s16.wav"))
    assert raw.sample_rate == 44100 and np.array_equal(raw.pcm[0], s16(44100))
    raw = A.decode_raw(str(corpus / "d_22k.flac"))
    assert raw.sample_rate == 22050 and raw.pcm.dtype == np.int16 and np.array_equal(raw.pcm[0], s16(22050))


@pytest.mark.parametrize("name", ["a_44k_s16.wav", "e_8k_u8.wav"])
def test_encode_resample_file_is_the_whole_files_encode(tok, resampler, corpus, name):
    path = Path(corpus / name)
    wav, want = whole_file_tokens(tok, resampler, path)
    got = tok.encode(path, chunk_size=1, stream=True, resample="file")
    assert got.shape == want.shape == (1, 8, -(-wav.shape[1] // HOP))
    assert torch.equal(got, want), f"{int((got != want).sum())} ids differ from encode of the whole-signal waveform"
    seams = tok.encode(path, chunk_size=1, stream=True)           # the default: every chunk resampled on its own
    print(f"{name}: resample='chunk' differs from the whole file in {int((seams != want).sum())} of {want.numel()} ids")


def ragged(total, seed):
    rng = np.random.default_rng(seed)
    sizes, left = [], total
    while left:
        s = min(left, int(rng.integers(1, 12000)))
        sizes.append(s)
        left -= s
    return sizes


def test_live_stream_at_its_own_rate(tok, resampler):
    pcm, code, scale, wav = whole_signal(resampler, 44100, "s16")
    ref = tok.stream()
    want = torch.cat([ref.push(wav[None]), ref.flush()], dim=-1)
    st = tok.stream(sample_rate=44100)
    x = torch.from_numpy(s16(44100))[None]
    parts, pos = [], 0
    for i, s in enumerate(ragged(x.shape[1], 5)):
        piece = x[:, pos:pos + s]
        parts.append(st.push(piece.numpy() if i % 2 else piece))      # int16, numpy and torch in turn
        pos += s
    parts.append(st.flush())
    got = torch.cat(parts, dim=-1)
    assert got.shape == want.shape and torch.equal(got, want), f"{int((got != want).sum())} ids differ from stream() fed the resampled waveform"
    assert torch.equal(got.cpu(), tok.encode(wav[None].cpu()))


def test_pool_with_streams_of_two_rates(tok, resampler):
    wav48 = whole_signal(resampler, 48000, "s16")[3]
    wav16 = whole_signal(resampler, 16000, "f32")[3]
    want = {}
    for key, wav in (("a", wav48), ("b", wav16)):
        ref = tok.stream()
        want[key] = torch.cat([ref.push(wav[None]), ref.flush()], dim=-1)[0]
    pool = tok.stream_pool(2)
    rs = tok.encoder.resampler()
    a, b = pool.open(sample_rate=48000), pool.open(sample_rate=16000)
    xa, xb = torch.from_numpy(s16(48000)), torch.from_numpy(X.signal(16000).copy())
    got = {a: [], b: []}
    steps, before = 5, rs.launches
    for i in range(steps):
        out = pool.push({a: xa[i * len(xa) // steps:(i + 1) * len(xa) // steps], b: xb[i * len(xb) // steps:(i + 1) * len(xb) // steps]})
        for sid in (a, b):
            got[sid].append(out[sid])
    assert rs.launches == before + steps, "the two streams of a call share one resample launch"
    fin = pool.flush([a, b])
    assert torch.equal(torch.cat(got[a] + [fin[a]], dim=-1), want["a"]) and torch.equal(torch.cat(got[b] + [fin[b]], dim=-1), want["b"])


def test_encode_batch_files_resample_file(tok, resampler, corpus, tmp_path):
    out = tmp_path / "tokens"
    tok.encode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=2, audio_dir=corpus, stream=True, resample="file")
    assert tok.skipped_files == []
    summary = dict(tok.run_summary)
    names = {"a_44k_s16.wav": "a_44k_s16.npy", "b_48k_f32.wav": "b_48k_f32.npy", "c_24k_s16.wav": "c_24k_s16.npy", "d_22k.flac": "d_22k.npy",
             "e_8k_u8.wav": "e_8k_u8.npy"}
    made = sorted(str(p.relative_to(out)) for p in out.rglob("*.npy"))
    assert len(made) == 7, made
    for src, npy in names.items():
        want = whole_file_tokens(tok, resampler, corpus / src)[1][0].numpy()
        got = np.load(out / npy)
        assert got.dtype == np.int16 and got.shape == want.shape and np.array_equal(got, want), f"{src}: {int((got != want).sum()) if got.shape == want.shape else 'shape'} differ"
    assert np.load(out / "b_48k_f32.npy").shape == (8, 75)
    # the tar's members: the tokens of the plain files they are copies of
    tar_npy = {os_path: np.load(out / os_path) for os_path in made if "in_tar" in os_path}
    assert len(tar_npy) == 2
    for p, got in tar_npy.items():
        twin = "a_44k_s16.npy" if "44k" in p else "d_22k.npy"
        assert np.array_equal(got, np.load(out / twin)), p
    # at the model's rate there is nothing to resample: the chunk route gives the same file
    chunked = tmp_path / "chunked"
    tok.encode_batch_files(batch_size=2, outdir=chunked, chunk_size=1, num_workers=0, audio_files=[corpus / "c_24k_s16.wav"], stream=True)
    assert np.array_equal(np.load(chunked / "c_24k_s16.npy"), np.load(out / "c_24k_s16.npy"))
    # one file at a time: ceil(seconds) chunk pushes and a final push each (none for the 1.0 s file, which ends on a frame) = 3 * 6 + 1 + 6 = 25; with two
    # slots the rows of a tick share pushes
    print(f"{summary['library_pushes']} library pushes, {summary['resample_launches']} resample launches, {summary}")
    assert summary["library_pushes"] < 25 and summary["resample_launches"] <= summary["library_pushes"]
