"""GPU: the streamed file drivers, encode_batch_files(stream=True) and decode_batch_files(stream=True).

What is asserted, and against what:
* every token file of the streamed run EQUALS what the facade's own B = 1 stream, encode(path, chunk_size, stream=True), returns for that file — the file is one
  clip, whichever files shared its pushes; the files longer than two chunks differ from the default (chunked) run's, which starts every chunk from a fresh LSTM;
* every audio file of the streamed decode EQUALS tests/pcm_ref.py (the one restatement of the float -> PCM rule) applied to decode(tokens, chunk_size,
  stream=True) of its token file, in clamp mode and with rescale=True, as WAV and as FLAC (read back by the package's own FLAC decoder).
"""
import os
import shutil
import wave
from pathlib import Path

import numpy as np
import pytest
import torch

from audiotoken_amd import audio_io as A
from audiotoken_amd import weights as W
from tests import pcm_ref as P

pytestmark = pytest.mark.gpu
HOP, SR = 320, 24000
FILES = {"half.wav": 12000, "one.wav": 24000, "spk/one_and_a_bit.wav": 24002, "spk/x/long.wav": int(2.7 * SR), "spk/x/longer.wav": int(3.3 * SR)}


@pytest.fixture(scope="module")
def weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True)


@pytest.fixture(scope="module")
def tok(cuda_device, weights):
    from audiotoken_amd import AudioToken, Tokenizers
    return AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=8, weights=weights)


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    from scipy.io import wavfile
    src = tmp_path_factory.mktemp("audio")
    (src / "spk" / "x").mkdir(parents=True)
    for i, (name, n) in enumerate(FILES.items()):
        wavfile.write(str(src / name), SR, np.round(W.synth_waveform(1, n, SR, seed=700 + i)[0] * 20000).astype(np.int16))
    return src


@pytest.fixture(scope="module")
def streamed_tokens(tok, corpus, tmp_path_factory):
    out = tmp_path_factory.mktemp("tokens")
    tok.encode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2, audio_dir=corpus, stream=True)
    assert tok.skipped_files == []
    return out


def _npy(name):
    return name[:-4] + ".npy"


def test_streamed_token_files_are_the_whole_files_tokens(tok, corpus, streamed_tokens, tmp_path):
    pushes = tok.run_summary["library_pushes"]
    chunked = tmp_path / "chunked"
    tok.encode_batch_files(batch_size=3, outdir=chunked, chunk_size=1, num_workers=2, audio_dir=corpus)      # the default route
    assert tok.skipped_files == []
    for name, n in FILES.items():
        got = np.load(streamed_tokens / _npy(name))                # the mirrored relative path
        want = tok.encode(Path(corpus / name), chunk_size=1, stream=True)
        assert want.shape == (1, 8, -(-n // HOP)) and got.dtype == np.int16
        assert got.shape == tuple(want.shape[1:]), name
        assert np.array_equal(got, want[0].numpy()), f"{name}: {int((got != want[0].numpy()).sum())} ids differ from encode(path, chunk_size=1, stream=True)"
        per_chunk = np.load(chunked / _npy(name))
        if n > 2 * SR:
            assert per_chunk.shape[0] == 8 and not np.array_equal(per_chunk[:, :got.shape[1]], got), f"{name}: the chunked run gave the whole file's tokens"
    # one file at a time: 1 + 1 + 1 + 3 + 4 chunk pushes (the 2-sample second chunk of the 24002-sample file is held) and 4 final pushes (the 1 s file ends on a
    # frame boundary) = 14; the pool shares them
    print(f"{pushes} library pushes for 5 files through 3 slots")
    assert pushes < 14


def test_an_undecodable_file_is_skipped_and_the_run_goes_on(tok, corpus, tmp_path):
    from scipy.io import wavfile
    src, out = tmp_path / "in", tmp_path / "out"
    src.mkdir()
    good = sorted(FILES)[:2]
    for i, name in enumerate(good):
        shutil.copy(corpus / name, src / f"{2 * i}_{os.path.basename(name)}")
    wavfile.write(str(src / "1_stereo.wav"), SR, np.zeros((SR, 2), dtype=np.int16))     # between the two good files
    (src / "3_garbage.wav").write_bytes(b"RIFF this is not a wave file")
    tok.encode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=0, audio_dir=src, stream=True)
    assert sorted(os.path.basename(p) for p, _ in tok.skipped_files) == ["1_stereo.wav", "3_garbage.wav"]
    assert sorted(os.listdir(out)) == [f"{2 * i}_{os.path.basename(n)[:-4]}.npy" for i, n in enumerate(good)]
    assert tok.run_summary["skipped_files"] == 2
    for i, name in enumerate(good):
        want = tok.encode(Path(corpus / name), chunk_size=1, stream=True)[0].numpy()
        assert np.array_equal(np.load(out / f"{2 * i}_{os.path.basename(name)[:-4]}.npy"), want)


def _read_wav(path):
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, SR)
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def _read_flac(path):
    raw = A.decode_raw(str(path))                    # the package's own reader: every CRC-8 / CRC-16 verified
    assert raw.sample_rate == SR and raw.pcm.shape[0] == 1 and raw.pcm.dtype == np.int16
    return raw.pcm[0]


_REF = {}


def _reference_audio(tok, streamed_tokens, name):
    """decode(tokens, chunk_size=1, stream=True) of a token file: float32 [320 T] from the B = 1 stream (computed once, shared by the four cases)."""
    if name not in _REF:
        t = torch.from_numpy(np.load(streamed_tokens / _npy(name)).astype(np.int64))
        _REF[name] = tok.decode(t, chunk_size=1, stream=True).numpy().ravel()
        assert _REF[name].shape == (HOP * t.shape[-1],)
    return _REF[name]


@pytest.mark.parametrize("rescale", (False, True), ids=("clamp", "rescale"))
@pytest.mark.parametrize("audio_format", ("wav", "flac"))
def test_streamed_decode_writes_the_pcm_of_the_streamed_clip(tok, streamed_tokens, tmp_path, audio_format, rescale):
    out = tmp_path / "audio"
    tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2, token_dir=streamed_tokens, rescale=rescale, audio_format=audio_format,
                           stream=True)
    assert tok.skipped_files == [] and tok.run_summary["files"] == len(FILES)
    for name in FILES:
        x = _reference_audio(tok, streamed_tokens, name)
        want, _, _ = P.quantise(x, P.file_scale(P.peak(x)) if rescale else 1.0)
        path = out / (name[:-4] + "." + audio_format)
        got = _read_wav(path) if audio_format == "wav" else _read_flac(path)
        assert len(got) == len(want), name
        diff = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print(f"{name} {audio_format} rescale={rescale}: {int((diff != 0).sum())} of {len(want)} samples differ, max {int(diff.max())} LSB")
        assert np.array_equal(got, want), f"{name}: {int((diff != 0).sum())} of {len(want)} samples differ from the B = 1 streamed decode (max {int(diff.max())} LSB)"
    print(f"{tok.run_summary['library_pushes']} library pushes in {tok.run_summary['batches']} ticks")
