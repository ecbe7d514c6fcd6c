"""CPU: the host side of decode_batch_files (audiotoken_amd/writer.py, audio_io.save_audio) — the segment planner, the WAV writer, the quantisation rule
against its restatement (tests/pcm_ref.py), token-file validation and the call errors. The file pipeline itself runs here with a stand-in decoder (a causal,
frame-local function of the tokens on the CPU) and ``device_writer=False``: the product's decoder and the device writer are the GPU file's business."""
import os
import struct
import wave

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd import audio_io as A
from audiotoken_amd import writer as Wr
from tests import pcm_ref as P

HOP = 320


# ---- the planner ---------------------------------------------------------------------------------------------------------------------------------------------
def _check_offsets(plan):
    """Row offsets and dst_off are contiguous: no gaps, no overlaps."""
    assert plan.t_max == max(7, max(r.valid for r in plan.rows))
    assert plan.src_off == [b * HOP * plan.t_max for b in range(len(plan.rows))]
    assert plan.n == [HOP * r.valid for r in plan.rows]
    pos = 0
    for b in range(len(plan.rows)):
        assert plan.dst_off[b] == pos
        assert plan.n[b] <= HOP * plan.t_max
        pos += plan.n[b]
    assert plan.total == pos


def test_planner_cuts_at_chunk_frames_and_fills_batches():
    plans = list(Wr.plan_batches([(0, 8, 2 * 150 + 40), (1, 8, 150)], batch_size=3, chunk_frames=Wr.chunk_frames_of(2)))
    assert Wr.chunk_frames_of(2) == 150 and Wr.chunk_frames_of(30) == 2250
    rows = [(r.file, r.t0, r.valid, r.last) for p in plans for r in p.rows]
    assert rows == [(0, 0, 150, False), (0, 150, 150, False), (0, 300, 40, True), (1, 0, 150, True)]
    assert [len(p.rows) for p in plans] == [3, 1] and all(p.K == 8 for p in plans)
    assert plans[0].t_max == 150
    for p in plans:
        _check_offsets(p)


def test_planner_pads_a_short_tail_to_seven_and_trims():
    (p,) = list(Wr.plan_batches([(0, 4, 3)], batch_size=8, chunk_frames=75))
    assert p.t_max == 7 and p.n == [3 * HOP] and p.src_off == [0] and p.dst_off == [0] and p.total == 3 * HOP
    toks = np.arange(12, dtype=np.int64).reshape(4, 3)
    batch = Wr.padded_tokens(p, lambda i: toks)
    assert batch.shape == (1, 4, 7) and batch.dtype == torch.int64
    assert torch.equal(batch[0, :, :3], torch.from_numpy(toks)) and bool((batch[0, :, 3:] == Wr.PAD_CODE).all()) and Wr.PAD_CODE < 0
    # a tail of 2 frames behind a full chunk: padded to the batch's longest row
    (p,) = list(Wr.plan_batches([(0, 8, 77)], batch_size=8, chunk_frames=75))
    assert [(r.t0, r.valid) for r in p.rows] == [(0, 75), (75, 2)] and p.t_max == 75 and p.n == [75 * HOP, 2 * HOP]
    _check_offsets(p)


def test_planner_closes_a_batch_when_k_changes():
    plans = list(Wr.plan_batches([(0, 8, 10), (1, 2, 10), (2, 2, 10), (3, 8, 10)], batch_size=16, chunk_frames=75))
    assert [(p.K, [r.file for r in p.rows]) for p in plans] == [(8, [0]), (2, [1, 2]), (8, [3])]
    for p in plans:
        _check_offsets(p)


def test_planner_without_chunking_gives_one_segment_per_file():
    plans = list(Wr.plan_batches([(0, 8, 5000), (1, 8, 20)], batch_size=4, chunk_frames=Wr.chunk_frames_of(None)))
    assert len(plans) == 1 and [(r.file, r.t0, r.valid, r.last) for r in plans[0].rows] == [(0, 0, 5000, True), (1, 0, 20, True)]
    assert plans[0].t_max == 5000
    _check_offsets(plans[0])


def test_planner_offsets_are_contiguous_on_ragged_input():
    rng = np.random.default_rng(3)
    files = [(i, int(rng.choice([2, 8])), int(rng.integers(1, 400))) for i in range(40)]
    seen = {}
    for p in Wr.plan_batches(files, batch_size=5, chunk_frames=60):
        assert 1 <= len(p.rows) <= 5
        _check_offsets(p)
        for r in p.rows:
            assert dict((f, k) for f, k, _ in files)[r.file] == p.K
            assert r.t0 == seen.get(r.file, 0)          # segments of a file in order, back to back
            seen[r.file] = r.t0 + r.valid
    assert seen == {i: T for i, _, T in files}


# ---- the WAV writer ---------------------------------------------------------------------------------------------------------------------------------------------
def test_wav_writer_write_patch_close_and_read_back(tmp_path):
    path = tmp_path / "sub" / "a.wav"
    x = (np.arange(-700, 700, dtype=np.int32) * 46).astype(np.int16)
    w = Wr.WavWriter(path, 24000)
    w.write(x[:500])
    w.write(x[500:].tobytes())
    assert not path.exists()            # nothing under the final name before close
    w.close()
    assert os.listdir(path.parent) == ["a.wav"]
    raw = path.read_bytes()
    assert len(raw) == 44 + 2 * len(x)
    assert struct.unpack("<I", raw[4:8])[0] == 36 + 2 * len(x) and struct.unpack("<I", raw[40:44])[0] == 2 * len(x)
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate(), f.getnframes()) == (1, 2, 24000, len(x))
        assert np.array_equal(np.frombuffer(f.readframes(len(x)), dtype="<i2"), x)
    dtype, sr, off, nbytes, scale, offset = A.wav_probe(str(path))
    assert (dtype, sr, off, nbytes, scale, offset) == (np.dtype("<i2"), 24000, 44, 2 * len(x), 1.0 / 32768.0, 0.0)
    back = A.read_audio(str(path), 24000)
    assert back.shape == (1, len(x)) and np.array_equal(back[0].numpy(), x.astype(np.float32) / np.float32(32768.0))


def test_wav_writer_overwrites_and_an_interrupted_writer_leaves_nothing(tmp_path):
    path = tmp_path / "a.wav"
    for n in (900, 100):                 # the second run REPLACES the first file: shorter, not appended
        w = Wr.WavWriter(path, 24000)
        w.write(np.full(n, n, dtype=np.int16))
        w.close()
    with wave.open(str(path), "rb") as f:
        assert f.getnframes() == 100
    before = path.read_bytes()
    w = Wr.WavWriter(path, 24000)
    w.write(np.zeros(5000, dtype=np.int16))
    w.abort()                            # interrupted: no partial file, and the complete file of the earlier run is untouched
    assert os.listdir(tmp_path) == ["a.wav"] and path.read_bytes() == before
    fresh = tmp_path / "b.wav"
    w = Wr.WavWriter(fresh, 24000)
    w.write(np.zeros(10, dtype=np.int16))
    w.abort()
    assert os.listdir(tmp_path) == ["a.wav"]


def test_wav_writer_refuses_to_pass_four_gib(tmp_path, monkeypatch):
    monkeypatch.setattr(Wr, "WAV_MAX_DATA", 1000)
    w = Wr.WavWriter(tmp_path / "big.wav", 24000)
    w.write(np.zeros(400, dtype=np.int16))
    with pytest.raises(Wr.WavTooLarge):
        w.write(np.zeros(200, dtype=np.int16))
    w.abort()
    assert os.listdir(tmp_path) == []


# ---- save_audio against the restatement ----------------------------------------------------------------------------------------------------------------------
def _hard_cases():
    k = np.array([-32440, -32439, -20001, -3, -2, -1, 0, 1, 2, 3, 7, 12344, 20000, 32438, 32439], dtype=np.float32)
    halves = (k + np.float32(0.5)) / np.float32(32768.0)            # exactly half-way between two codes: ties go to the even one
    rng = np.random.default_rng(11)
    body = rng.standard_normal(4000).astype(np.float32) * np.float32(0.6)          # some beyond +-0.99
    edge = np.array([0.99, -0.99, np.nextafter(np.float32(0.99), np.float32(2)), np.nextafter(np.float32(-0.99), np.float32(-2)), 1.0, -1.0, 1.5, -6.25,
                     3.4e38, -3.4e38, 1e-45, -0.0, 0.0, np.nan, np.inf, -np.inf], dtype=np.float32)
    return np.concatenate([halves, body, edge, halves * np.float32(3.0)]).astype(np.float32)


@pytest.mark.parametrize("rescale", [False, True])
def test_save_audio_equals_the_restatement(tmp_path, rescale):
    x = _hard_cases()
    path = tmp_path / "x.wav"
    clipped, nonfinite = A.save_audio(torch.from_numpy(x)[None], path, 24000, rescale=rescale)
    scale = P.file_scale(P.peak(x)) if rescale else np.float32(1.0)
    want, want_clipped, want_nonfinite = P.quantise(x, scale)
    with wave.open(str(path), "rb") as f:
        got = np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")
        assert f.getframerate() == 24000 and f.getnchannels() == 1
    assert np.array_equal(got, want)
    assert (clipped, nonfinite) == (want_clipped, want_nonfinite) and nonfinite == 3
    assert np.abs(got.astype(np.int32)).max() <= 32440
    assert (scale < 1) if rescale else (clipped > 100)         # the finite peak (3.4e38) sets the scale
    # ties to even, stated independently of numpy's rint: (k + 0.5) / 32768 -> the even neighbour
    ties, _, _ = A.pcm16_from_float((np.array([0, 1, 2, 3, -1, -2, -3], dtype=np.float32) + np.float32(0.5)) / np.float32(32768.0))
    assert ties.tolist() == [0, 2, 2, 4, 0, -2, -2]


def test_save_audio_within_range_scale_is_one_and_arrays_work(tmp_path):
    x = np.linspace(-0.5, 0.5, 1001, dtype=np.float32)
    A.save_audio(x, tmp_path / "a.wav", 16000, rescale=True)       # peak 0.5: min(0.99 / 0.5, 1) = 1, nothing is amplified
    A.save_audio(x, tmp_path / "b.wav", 16000, rescale=False)
    assert (tmp_path / "a.wav").read_bytes() == (tmp_path / "b.wav").read_bytes()
    from audiotoken_amd import save_audio
    assert save_audio is A.save_audio
    with pytest.raises(ValueError):
        A.save_audio(np.zeros((2, 10), np.float32), tmp_path / "c.wav", 16000)


# ---- the file pipeline with a stand-in decoder ----------------------------------------------------------------------------------------------------------------
class _StubDecoder:
    """Causal and frame-local: sample j of frame t depends on the codes of frame t only, so right padding cannot change earlier samples. Peak ~ 2.6."""
    fallback_batches = 0

    def __init__(self, fail_at=None):
        self.calls, self.fail_at = [], fail_at

    def forward(self, toks):
        B, K, T = toks.shape
        self.calls.append((B, K, T))
        if self.fail_at is not None and len(self.calls) == self.fail_at:
            raise RuntimeError("stand-in device failure")
        base = (toks.to(torch.float32) * torch.arange(1, K + 1, dtype=torch.float32)[None, :, None]).sum(1) / (K * 600.0) - 0.8      # [B, T]
        ramp = torch.arange(HOP, dtype=torch.float32) / HOP
        return (base[:, :, None] * (1.0 + ramp)[None, None, :]).reshape(1, B * HOP * T)

    def verified(self, wav, toks):
        return wav


def _tok(decoder=None):
    t = AudioToken(Tokenizers.acoustic, device="cpu", num_codebooks=8)
    t.decoder = decoder or _StubDecoder()
    return t


def _tokens(K, T, seed):
    return np.random.default_rng(seed).integers(0, 1024, size=(K, T)).astype(np.int64)


def _expected(stub_tokens, rescale, chunk_frames):
    K, T = stub_tokens.shape
    step = T if chunk_frames is None else chunk_frames
    x = np.concatenate([_StubDecoder().forward(torch.from_numpy(stub_tokens[None, :, t0:t0 + step])).numpy().ravel() for t0 in range(0, T, step)])
    return P.quantise(x, P.file_scale(P.peak(x)) if rescale else 1.0)


def _read(path):
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 24000)
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


@pytest.mark.parametrize("rescale", [False, True])
def test_pipeline_writes_the_tree_and_matches_the_restatement(tmp_path, rescale):
    src, out = tmp_path / "tokens", tmp_path / "wav"
    (src / "deep" / "er").mkdir(parents=True)
    (src / ".hidden").mkdir()
    toks = {"a.npy": _tokens(8, 2 * 75 + 9, 1), "b.npy": _tokens(8, 3, 2), "c.npy": _tokens(2, 80, 3), "d.npy": _tokens(8, 75, 4),
            "deep/er/e.npy": _tokens(8, 5 * 75, 5)}
    for name, t in toks.items():
        np.save(src / name, t.astype(np.int16) if name == "a.npy" else (t[None] if name == "d.npy" else t))
    np.save(src / ".hidden" / "x.npy", _tokens(8, 10, 6))
    np.save(src / ".dot.npy", _tokens(8, 10, 7))
    (src / "notes.txt").write_text("not a token file")
    stub = _StubDecoder()
    tok = _tok(stub)
    tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2, token_dir=src, rescale=rescale, device_writer=False)
    assert tok.skipped_files == []
    found = sorted(os.path.relpath(os.path.join(d, n), out) for d, _, names in os.walk(out) for n in names)
    assert found == ["a.wav", "b.wav", "c.wav", "d.wav", "deep/er/e.wav"]
    clipped = 0
    for name, t in toks.items():
        want, c, _ = _expected(t, rescale, 75)
        clipped += c
        got = _read(out / (name[:-4] + ".wav"))
        assert len(got) == HOP * t.shape[1] and np.array_equal(got, want), name
    # a(3 rows) | b | c (K = 2 closes the batch on both sides) | d, e0, e1 | e2..e4: a file that spans batches keeps its order and, with rescale, ONE scale
    assert [(B, K) for B, K, _ in stub.calls] == [(3, 8), (1, 8), (2, 2), (3, 8), (3, 8)]
    assert stub.calls[1][2] == 7                                    # the 3-frame file is padded to the decoder's 7
    s = tok.run_summary
    assert (s["files"], s["segments"], s["batches"], s["fallback_batches"], s["skipped_files"], s["nonfinite_samples"]) == (5, 12, 5, 0, 0, 0)
    assert s["clipped_samples"] == clipped and (rescale or clipped > 1000)
    for key in ("stage_s", "encode_call_s", "device_wait_s", "save_s", "batches", "rows", "total_s"):
        assert key in tok.run_timings
    # a second run over the same tree overwrites: same bytes, not twice the audio
    before = (out / "a.wav").read_bytes()
    tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=0, token_dir=src, rescale=rescale, device_writer=False)
    assert (out / "a.wav").read_bytes() == before


def test_validation_reasons_and_the_run_goes_on(tmp_path):
    src, out = tmp_path / "t", tmp_path / "o"
    src.mkdir()
    (src / "sub").mkdir()
    good = _tokens(8, 20, 1)
    np.save(src / "good1.npy", good)
    np.save(src / "rank.npy", _tokens(8, 20, 2).reshape(2, 4, 20))
    np.save(src / "rank1.npy", np.arange(20, dtype=np.int64))
    np.save(src / "toomany.npy", _tokens(9, 20, 3))
    hi = _tokens(8, 20, 4); hi[3, 7] = 1024
    np.save(src / "hi.npy", hi)
    lo = _tokens(8, 20, 5); lo[0, 0] = -1
    np.save(src / "lo.npy", lo.astype(np.int16))
    np.save(src / "empty.npy", np.zeros((8, 0), dtype=np.int64))
    np.save(src / "floats.npy", np.zeros((8, 5), dtype=np.float32))
    (src / "text.npy").write_text("this is not numpy")
    (src / "notes.txt").write_text("nor is this")
    np.save(src / "sub" / "good1.npy", good)                        # maps to the same flat output name as the first
    np.save(src / "good2.npy", _tokens(4, 9, 6))
    names = ["good1.npy", "rank.npy", "rank1.npy", "toomany.npy", "hi.npy", "lo.npy", "empty.npy", "floats.npy", "text.npy", "notes.txt", "sub/good1.npy",
             "good2.npy"]
    tok = _tok()
    tok.decode_batch_files(batch_size=4, outdir=out, chunk_size=30, num_workers=3, token_files=[src / n for n in names], device_writer=False)
    reasons = {os.path.relpath(p, src): why for p, why in tok.skipped_files}
    assert sorted(reasons) == sorted(n for n in names if n not in ("good1.npy", "good2.npy"))
    assert "rank 3" in reasons["rank.npy"] and "rank 1" in reasons["rank1.npy"]
    assert "9 code books" in reasons["toomany.npy"] and "the model has 8" in reasons["toomany.npy"]
    assert "code 1024 outside [0, 1023]" in reasons["hi.npy"]
    assert "code -1 outside [0, 1023]" in reasons["lo.npy"]
    assert "empty token file" in reasons["empty.npy"]
    assert "dtype float32" in reasons["floats.npy"]
    assert "unreadable token file" in reasons["text.npy"] and "unreadable token file" in reasons["notes.txt"]
    assert "duplicate output name" in reasons["sub/good1.npy"]
    assert sorted(os.listdir(out)) == ["good1.wav", "good2.wav"]      # flat, and the run went on past every skip
    assert np.array_equal(_read(out / "good1.wav"), _expected(good, False, 2250)[0])
    assert tok.run_summary["files"] == 2 and tok.run_summary["skipped_files"] == len(names) - 2
    # in directory mode only .npy files are inputs, and the two good1 files no longer collide
    tok.decode_batch_files(batch_size=4, outdir=tmp_path / "o2", chunk_size=30, num_workers=0, token_dir=src, device_writer=False)
    assert "notes.txt" not in {os.path.relpath(p, src) for p, _ in tok.skipped_files}
    assert (tmp_path / "o2" / "sub" / "good1.wav").exists() and (tmp_path / "o2" / "good1.wav").exists()


def test_a_failing_batch_leaves_complete_files_or_none(tmp_path):
    src, out = tmp_path / "t", tmp_path / "o"
    src.mkdir()
    np.save(src / "a.npy", _tokens(8, 75, 1))
    np.save(src / "b.npy", _tokens(8, 3 * 75, 2))       # rows in batches 1 and 2: the second decode call fails
    tok = _tok(_StubDecoder(fail_at=2))
    with pytest.raises(RuntimeError, match="stand-in device failure"):
        tok.decode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=0, token_dir=src, device_writer=False)
    assert os.listdir(out) == ["a.wav"]                 # a is complete and closed; b was open and is removed, no .part is left
    assert np.array_equal(_read(out / "a.wav"), _expected(_tokens(8, 75, 1), False, 75)[0])
    assert tok.run_summary["files"] == 1


def test_rescale_hold_is_bounded(tmp_path):
    src, out = tmp_path / "t", tmp_path / "o"
    src.mkdir()
    np.save(src / "a.npy", _tokens(8, 6 * 75, 1))       # 6 rows of 75 frames = 6 x 96 000 held bytes
    np.save(src / "b.npy", _tokens(8, 75, 2))
    tok = _tok()
    tok.decode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=0, token_dir=src, rescale=True, device_writer=False,
                           max_held_bytes=4 * 96000)
    assert [os.path.basename(p) for p, _ in tok.skipped_files] == ["a.npy"] and "max_held_bytes" in tok.skipped_files[0][1]
    assert os.listdir(out) == ["b.wav"]
    assert np.array_equal(_read(out / "b.wav"), _expected(_tokens(8, 75, 2), True, 75)[0])


# ---- call errors --------------------------------------------------------------------------------------------------------------------------------------------------
def test_call_errors(tmp_path):
    tok = _tok()
    with pytest.raises(AssertionError, match="Either token_files or token_dir"):
        tok.decode_batch_files(batch_size=2, outdir=tmp_path / "o")
    with pytest.raises(AssertionError, match="not both"):
        tok.decode_batch_files(batch_size=2, outdir=tmp_path / "o", token_files=[tmp_path / "a.npy"], token_dir=tmp_path)
    for name in (Tokenizers.semantic_s, Tokenizers.semantic_m):
        sem = AudioToken(name, device="cuda:0")
        with pytest.raises(NotImplementedError):          # what load_decoder raises for a tokenizer without a decoder
            sem.decode_batch_files(batch_size=2, outdir=tmp_path / "o", token_dir=tmp_path)


# ---- the C ABI of the device writer: arguments are validated without touching the device ----------------------------------------------------------------------
def test_pcm_entry_points_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    assert C.sizeof(_cabi.PcmRowDesc) == 32
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)            # never dereferenced: every call below is refused by its argument check
    for bad in (lambda: lib.at_pcm_pack(None, p, 1, 8, 0.99, p, p, None), lambda: lib.at_pcm_pack(p, None, 1, 8, 0.99, p, p, None),
                lambda: lib.at_pcm_pack(p, p, 1, 8, 0.99, None, p, None), lambda: lib.at_pcm_pack(p, p, 1, 8, 0.99, p, None, None),
                lambda: lib.at_pcm_pack(p, p, -1, 8, 0.99, p, p, None), lambda: lib.at_pcm_pack(p, p, 1, -8, 0.99, p, p, None)):
        assert bad() != 0 and "at_pcm_pack: bad arguments" in _cabi.last_error()
    for limit in (0.0, -0.5, 1.0, float("nan")):
        assert lib.at_pcm_pack(p, p, 1, 8, limit, p, p, None) != 0 and "limit" in _cabi.last_error()
    assert lib.at_pcm_pack(p, p, 1 << 30, 1 << 40, 0.99, p, p, None) != 0 and "tiles" in _cabi.last_error()
    for bad in (lambda: lib.at_pcm_peaks(None, p, 1, 8, p, None), lambda: lib.at_pcm_peaks(p, None, 1, 8, p, None),
                lambda: lib.at_pcm_peaks(p, p, 1, 8, None, None), lambda: lib.at_pcm_peaks(p, p, -1, 8, p, None),
                lambda: lib.at_pcm_peaks(p, p, 1, -1, p, None)):
        assert bad() != 0 and "at_pcm_peaks: bad arguments" in _cabi.last_error()
    assert lib.at_pcm_pack(p, p, 0, 0, 0.99, p, p, None) == 0 and lib.at_pcm_peaks(p, p, 0, 0, p, None) == 0      # no rows: nothing to do
