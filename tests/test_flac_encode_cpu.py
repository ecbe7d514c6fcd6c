"""CPU: the FLAC output path without a device — the host twin of the encoder (at_flac_encode_pcm16), the framing (at_flac_write_frames, at_flac_streaminfo),
``FlacWriter`` and ``save_audio``.

What is asserted, and against what:
1. for every signal and every length of tests/flac_enc_ref.py: the file the library writes EQUALS the restatement's file, byte for byte; the library's own
   FLAC decoder (which verifies every CRC-8 / CRC-16 itself) returns exactly the int16 samples; at_flac_info returns rate, bit depth, channels and total;
2. coverage, on the restatement alone: the chosen subframes include CONSTANT, VERBATIM, FIXED of every order 0..4, partition orders 0 and 6, a partition with
   k = 0 and one with k >= 12;
3. ``FlacWriter``: a complete file or nothing at ``path``; ``abort`` leaves no ``.part``;
4. ``save_audio``: ``x.flac`` round-trips through ``read_audio``; ``x.wav`` and extension-less paths write the bytes they wrote before;
5. ``decode_batch_files(audio_format="ogg")`` raises ValueError.
"""
import ctypes as C
import os

import numpy as np
import pytest

from audiotoken_amd import _cabi
from audiotoken_amd import audio_io as A
from audiotoken_amd import writer as Wr
from tests import flac_enc_ref as F
from tests import pcm_ref as P


def _library_file(rows, sample_rate, path):
    w = Wr.FlacWriter(path, sample_rate)
    recs, data = Wr.flac_encode_pcm16(rows)
    for j in range(len(rows)):
        first = np.zeros(len(rows), dtype=np.int64)
        first[j] = w.samples
        w.write(*Wr.flac_frames(recs[recs["row"] == j], data, sample_rate, first))
    w.close()
    with open(path, "rb") as f:
        return f.read(), recs


def _decode(blob):
    lib = _cabi.load()
    sr, ch, bits, total = C.c_int(), C.c_int(), C.c_int(), C.c_int64()
    buf = np.frombuffer(blob, dtype=np.uint8)
    assert lib.at_flac_info(buf.ctypes.data, len(blob), C.byref(sr), C.byref(ch), C.byref(bits), C.byref(total), None) == 0, _cabi.last_error()
    out = np.empty((1, max(total.value, 1)), dtype=np.int32)
    n = lib.at_flac_decode(buf.ctypes.data, len(blob), out.ctypes.data, out.shape[1])
    assert n == total.value, _cabi.last_error()
    return out[0, :n], (sr.value, ch.value, bits.value, total.value)


@pytest.fixture(scope="module")
def reference_files():
    """{(signal, n): (file bytes, block info)} of the restatement, computed once."""
    return {(name, n): F.encode_rows([F.signal(name, n)]) for name in F.SIGNALS for n in F.LENGTHS}


@pytest.mark.parametrize("name", F.SIGNALS)
def test_host_twin_and_framing_equal_the_restatement(name, reference_files, tmp_path):
    for n in F.LENGTHS:
        q = F.signal(name, n)
        assert np.abs(q).max() <= 32440
        want, info = reference_files[(name, n)]
        got, recs = _library_file([q.astype(np.int16)], 24000, str(tmp_path / f"{n}.flac"))
        assert [(int(r["first"]), int(r["n"]), int(r["kind"]), int(r["order"]), int(r["porder"]), int(r["nbytes"])) for r in recs] == \
               [(a, bn, kind, o, p, len(sub)) for _, a, bn, kind, o, p, _, sub in info], f"{name} n={n}: block records"
        assert got == want, f"{name} n={n}: the library's file differs from the restatement's"
        samples, meta = _decode(got)
        assert np.array_equal(samples, q), f"{name} n={n}: the decoder does not return the samples"
        assert meta == (24000, 1, 16, n)


def test_host_twin_equals_the_restatement_where_partitions_differ(tmp_path):
    """A tone under bursts of noise: partition orders 5 and 6 with Rice parameters from 4 to 14 inside one block."""
    rows = [F.bursts(n, j) for j, n in enumerate((4097, 1408, 2240, 4095))]
    want, info = F.encode_rows(rows)
    assert {5, 6} <= {p for *_, kind, _, p, _, _ in info if kind == F.FIXED} and len({k for x in info for k in x[6]}) >= 8
    got, _ = _library_file([r.astype(np.int16) for r in rows], 24000, str(tmp_path / "b.flac"))
    assert got == want
    assert np.array_equal(_decode(got)[0], np.concatenate(rows))


def test_restatement_covers_every_subframe_kind(reference_files):
    kinds, orders, porders, ks = set(), set(), set(), set()
    for _, info in reference_files.values():
        for _, _, _, kind, o, p, kk, _ in info:
            kinds.add(kind)
            if kind == F.FIXED:
                orders.add(o); porders.add(p); ks.update(kk)
    assert kinds == {F.CONSTANT, F.VERBATIM, F.FIXED}
    assert orders == {0, 1, 2, 3, 4}, orders
    assert 0 in porders and 6 in porders, porders
    assert 0 in ks and max(ks) >= 12, ks


def test_rows_are_independent_and_sample_numbers_run_on(tmp_path):
    """Three rows in one file (as the segments of decode_batch_files), another rate, and a coded number beyond 2^31 (7 bytes)."""
    rows = [F.signal("sine_a16", 4160), F.signal("uniform_pm3", 64), F.signal("sine_a256", 2240)]
    want, _ = F.encode_rows(rows, 16000)
    got, _ = _library_file([r.astype(np.int16) for r in rows], 16000, str(tmp_path / "rows.flac"))
    assert got == want
    samples, meta = _decode(got)
    assert np.array_equal(samples, np.concatenate(rows)) and meta == (16000, 1, 16, 4160 + 64 + 2240)
    recs, data = Wr.flac_encode_pcm16([rows[1].astype(np.int16)])
    frames, stats = Wr.flac_frames(recs, data, 12345, [(1 << 35) + 7])
    sub, *_ = F.subframe(rows[1])
    assert bytes(frames) == F.frame(sub, 64, (1 << 35) + 7, 12345) and int(stats[6]) == 64


def test_framing_rejects_damaged_records():
    lib = _cabi.load()
    recs, data = Wr.flac_encode_pcm16([F.signal("sine_a16", 100).astype(np.int16)])
    bad = recs.copy()
    bad["byte_off"][0] = len(data)
    with pytest.raises(_cabi.HipLibraryError, match="outside the subframe bytes"):
        Wr.flac_frames(bad, data, 24000, [0])
    with pytest.raises(_cabi.HipLibraryError, match="2\\^36"):
        Wr.flac_frames(recs, data, 24000, [(1 << 36) - 50])
    head = (C.c_uint8 * 42)()
    assert lib.at_flac_streaminfo(24000, 4096, 4096, 10, 20, 1 << 36, head) != 0 and "2^36" in _cabi.last_error()
    assert lib.at_flac_encode_pcm16(None, 5, 0, recs.ctypes.data, 1, data.ctypes.data, 100, 0) < 0
    q = np.zeros(5000, np.int16)
    assert lib.at_flac_encode_pcm16(q.ctypes.data, 5000, 0, recs.ctypes.data, 1, data.ctypes.data, 1 << 20, 0) < 0 and "blocks_cap" in _cabi.last_error()


def test_flac_writer_leaves_a_complete_file_or_nothing(tmp_path):
    path = tmp_path / "deep" / "x.flac"
    recs, data = Wr.flac_encode_pcm16([F.signal("sine_a16", 5000).astype(np.int16)])
    frames, stats = Wr.flac_frames(recs, data, 24000, [0])
    w = Wr.FlacWriter(path, 24000)
    w.write(frames, stats)
    assert not path.exists() and os.path.exists(str(path) + ".part")
    w.abort()
    assert not path.exists() and not os.path.exists(str(path) + ".part")
    path.write_bytes(b"an earlier file")
    w = Wr.FlacWriter(path, 24000)
    w.write(frames, stats)
    assert path.read_bytes() == b"an earlier file"
    w.abort()
    assert path.read_bytes() == b"an earlier file" and not os.path.exists(str(path) + ".part")
    w = Wr.FlacWriter(path, 24000)
    w.write(frames, stats)
    w.close()
    assert not os.path.exists(str(path) + ".part")
    assert path.read_bytes() == F.encode_rows([F.signal("sine_a16", 5000)])[0] and w.data_bytes == len(path.read_bytes())


def test_save_audio_flac_round_trips_and_wav_is_unchanged(tmp_path):
    import torch
    rng = np.random.default_rng(3)
    x = (rng.standard_normal(7001) * 0.5).astype(np.float32)
    x[[5, 77, 900]] = [np.nan, np.inf, -np.inf]
    for rescale in (False, True):
        scale = P.file_scale(P.peak(x)) if rescale else np.float32(1.0)
        q, clipped, nonfinite = P.quantise(x, scale)
        assert A.save_audio(torch.from_numpy(x)[None], tmp_path / "x.flac", 24000, rescale=rescale) == (clipped, nonfinite)
        assert (tmp_path / "x.flac").read_bytes() == F.encode_rows([q])[0]
        back = A.read_audio(str(tmp_path / "x.flac"), 24000)
        assert back.shape == (1, len(x)) and np.array_equal(back[0].numpy(), q.astype(np.float32) / np.float32(32768.0))
        # WAV: the bytes of before — RIFF header + the restatement's samples; an extension-less path is WAV as well
        wav_bytes = (b"RIFF" + (36 + 2 * len(q)).to_bytes(4, "little") + b"WAVEfmt " + (16).to_bytes(4, "little") + (1).to_bytes(2, "little")
                     + (1).to_bytes(2, "little") + (24000).to_bytes(4, "little") + (48000).to_bytes(4, "little") + (2).to_bytes(2, "little")
                     + (16).to_bytes(2, "little") + b"data" + (2 * len(q)).to_bytes(4, "little") + q.astype("<i2").tobytes())
        for name in ("x.wav", "noext"):
            assert A.save_audio(x, tmp_path / name, 24000, rescale=rescale) == (clipped, nonfinite)
            assert (tmp_path / name).read_bytes() == wav_bytes, name
    A.save_audio(x, tmp_path / "forced", 24000, audio_format="flac")
    assert (tmp_path / "forced").read_bytes()[:4] == b"fLaC"
    with pytest.raises(ValueError):
        A.save_audio(x, tmp_path / "y.ogg", 24000, audio_format="ogg")


def test_output_path_takes_the_format():
    assert Wr.output_path("/t/sub/a.npy", "/o", "/t", "flac") == os.path.join("/o", "sub", "a.flac")
    assert Wr.output_path("/t/sub/a.npy", "/o", "/t") == os.path.join("/o", "sub", "a.wav")


def test_decode_batch_files_refuses_an_unknown_format(tmp_path):
    from audiotoken_amd import AudioToken, Tokenizers
    tok = AudioToken.__new__(AudioToken)          # the check comes before anything of the instance is read: no decoder is loaded
    tok.tokenizer_name = Tokenizers.acoustic
    with pytest.raises(ValueError, match="audio_format"):
        tok.decode_batch_files(batch_size=1, outdir=tmp_path, token_dir=tmp_path, audio_format="ogg")
    assert not hasattr(tok, "decoder") or tok.decoder is None
