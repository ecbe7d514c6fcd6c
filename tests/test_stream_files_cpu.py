"""CPU: the streamed file drivers, encode_batch_files(stream=True) and decode_batch_files(stream=True), over stand-in models whose stream pools are the real
pool classes with stub device calls (tests/test_stream_pool_cpu.py: the state of a stream is one counter, its number of frames so far).

Encode: code 0 of a frame is the frame's index by the carried state, code 1 the frame's first sample, so a token file is right only if the file was ONE
stream (state carried across its chunks, through whatever slots and groups) fed with its own samples in order.
Decode: the stand-in decoder of tests/test_decode_files_cpu.py is frame-local, so the streamed audio must equal its one-shot decode of the whole file; the
PCM is held to tests/pcm_ref.py.
"""
import os
import wave

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd import audio_io as A
from audiotoken_amd.streaming import AcousticDecodeStreamPool, AcousticStreamPool
from tests import pcm_ref as P
from tests.test_stream_pool_cpu import StubDevice

HOP, SR = 320, 24000


class _StubEncoder:
    fallback_batches = nonfinite_batches = 0

    def __init__(self):
        self.devices = []

    def new_stream_pool(self, slots):
        dev = StubDevice(slots)

        def push(x, final, started):
            codes = dev.push_encode(x, final, started)
            codes[:, 1] = torch.round(x[:, ::HOP][:, :codes.shape[-1]] * 1000).to(torch.int16)      # the frame's first sample, in thousandths
            return codes
        self.devices.append(dev)
        return AcousticStreamPool(None, slots, push_fn=push, gather_fn=dev.gather, scatter_fn=dev.scatter, n_q=2)


def _tok(encoder=None, decoder=None):
    t = AudioToken(Tokenizers.acoustic, device="cpu", num_codebooks=8)
    t.encoder, t.decoder = encoder, decoder
    return t


FILES = {"a.wav": 12000, "b.wav": 24000, "sub/c.wav": 24002, "sub/deep/d.wav": int(2.7 * SR), "sub/deep/e.wav": int(3.3 * SR), "f.wav": 400}


def _corpus(root):
    from scipy.io import wavfile
    (root / "sub" / "deep").mkdir(parents=True)
    for i, (name, n) in enumerate(sorted(FILES.items())):
        wavfile.write(str(root / name), SR, np.full(n, (i + 1) / 16.0, dtype=np.float32))      # a float32 WAV of one exactly representable value per file


def test_streamed_encode_driver_writes_each_files_own_stream(tmp_path):
    src, out = tmp_path / "audio", tmp_path / "tokens"
    _corpus(src)
    from scipy.io import wavfile
    wavfile.write(str(src / "bad_stereo.wav"), SR, np.zeros((SR, 2), dtype=np.int16))
    wavfile.write(str(src / "tiny.wav"), SR, np.zeros(300, dtype=np.float32))                    # below the 321 samples of a clip
    (src / "members.tar").write_bytes(b"")
    enc = _StubEncoder()
    tok = _tok(encoder=enc)
    tok.encode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2, audio_dir=src, stream=True)
    reasons = {os.path.basename(p): why for p, why in tok.skipped_files}
    assert sorted(reasons) == ["bad_stereo.wav", "members.tar", "tiny.wav"]
    assert "mono" in reasons["bad_stereo.wav"] and "archives are not streamed" in reasons["members.tar"] and "321" in reasons["tiny.wav"]
    found = sorted(os.path.relpath(os.path.join(d, n), out) for d, _, names in os.walk(out) for n in names)
    assert found == sorted(name[:-4] + ".npy" for name in FILES)                                 # the relative tree is kept
    for i, (name, n) in enumerate(sorted(FILES.items())):
        got = np.load(out / (name[:-4] + ".npy"))
        T = -(-n // HOP)
        assert got.shape == (2, T) and got.dtype == np.int16, name
        assert got[0].tolist() == list(range(T)), f"{name}: not one stream (frame indices by the carried state: {got[0].tolist()[:12]} ...)"
        assert set(got[1].tolist()) == {round(1000 * (i + 1) / 16.0)}, f"{name}: another file's samples"
    dev = enc.devices[-1]
    assert tok.run_summary["library_pushes"] == len(dev.pushes()) and tok.run_summary["skipped_files"] == 3
    assert max(e[1] for e in dev.pushes()) > 1, "no two files ever shared a push"
    assert tok.run_timings["rows"] == sum(-(-n // SR) for n in FILES.values())                  # one row per file and chunk
    # the same call without stream=True is the chunked route as before (it needs a real encoder: here it only must not take the streamed path)
    with pytest.raises(Exception):
        tok.encode_batch_files(batch_size=3, outdir=tmp_path / "x", chunk_size=1, num_workers=0, audio_files=[str(src / "a.wav")], device_feeder=False)


def test_streamed_encode_driver_with_a_file_list_appends_flat(tmp_path):
    src, out = tmp_path / "audio", tmp_path / "tokens"
    _corpus(src)
    tok = _tok(encoder=_StubEncoder())
    files = [str(src / "sub/deep/d.wav"), str(src / "a.wav")]
    tok.encode_batch_files(batch_size=1, outdir=out, chunk_size=1, num_workers=0, audio_files=files, stream=True)
    assert sorted(os.listdir(out)) == ["a.npy", "d.npy"] and tok.skipped_files == []
    assert np.load(out / "d.npy")[0].tolist() == list(range(-(-FILES["sub/deep/d.wav"] // HOP)))
    tok.encode_batch_files(batch_size=1, outdir=out, chunk_size=1, num_workers=0, audio_files=files[1:], stream=True)      # a second run appends, as ever
    assert np.load(out / "a.npy").shape == (2, 2 * 38)


# ---- decode ---------------------------------------------------------------------------------------------------------------------------------------------------
class _StubDecoder:
    """tests/test_decode_files_cpu.py's stand-in: frame-local, peak ~ 2.6; its pool pushes through the same arithmetic."""
    fallback_batches = 0

    def __init__(self):
        self.devices = []

    def forward(self, toks):
        B, K, T = toks.shape
        base = (toks.to(torch.float32) * torch.arange(1, K + 1, dtype=torch.float32)[None, :, None]).sum(1) / (K * 600.0) - 0.8      # [B, T]
        ramp = torch.arange(HOP, dtype=torch.float32) / HOP
        return (base[:, :, None] * (1.0 + ramp)[None, None, :]).reshape(1, B * HOP * T)

    def new_stream_pool(self, slots):
        dev = StubDevice(slots)

        def push(toks, started):
            dev.push_decode(toks, started)                       # the counter state and the log
            return self.forward(toks).reshape(toks.shape[0], -1)
        self.devices.append(dev)
        return AcousticDecodeStreamPool(None, slots, push_fn=push, gather_fn=dev.gather, scatter_fn=dev.scatter)


def _tokens(K, T, seed):
    return np.random.default_rng(seed).integers(0, 1024, size=(K, T)).astype(np.int64)


def _read_wav(path):
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, SR)
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


@pytest.mark.parametrize("audio_format", ("wav", "flac"))
@pytest.mark.parametrize("rescale", (False, True), ids=("clamp", "rescale"))
def test_streamed_decode_driver_matches_the_restatement(tmp_path, rescale, audio_format):
    src, out = tmp_path / "tokens", tmp_path / "audio"
    (src / "deep").mkdir(parents=True)
    toks = {"a.npy": _tokens(8, 2 * 75 + 9, 1), "b.npy": _tokens(8, 3, 2), "c.npy": _tokens(2, 80, 3), "d.npy": _tokens(8, 75, 4),
            "deep/e.npy": _tokens(8, 5 * 75, 5)}
    for name, t in toks.items():
        np.save(src / name, t.astype(np.int16) if name == "a.npy" else t)
    (src / "z_bad.npy").write_bytes(b"\x93NUMPY\x01\x00 this header never ends")
    dec = _StubDecoder()
    tok = _tok(decoder=dec)
    tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2, token_dir=src, rescale=rescale, device_writer=False,
                           audio_format=audio_format, stream=True)
    assert [os.path.basename(p) for p, _ in tok.skipped_files] == ["z_bad.npy"]
    clipped = 0
    for name, t in toks.items():
        x = dec.forward(torch.from_numpy(t[None])).numpy().ravel()                              # the file as ONE clip
        want, c, _ = P.quantise(x, P.file_scale(P.peak(x)) if rescale else 1.0)
        clipped += c
        path = out / (name[:-4] + "." + audio_format)
        got = _read_wav(path) if audio_format == "wav" else A.decode_raw(str(path)).pcm[0]
        assert len(got) == HOP * t.shape[1] and np.array_equal(got, want), name
    s = tok.run_summary
    # ticks: (a0 b c0) (a1 c1 d) (a2 e0) e1 e2 e3 e4 — a file's place goes to the next file when it ends
    assert (s["files"], s["segments"], s["batches"], s["skipped_files"], s["clipped_samples"]) == (5, 12, 7, 1, clipped)
    dev = dec.devices[-1]
    assert s["library_pushes"] == len(dev.pushes())
    assert dev.pushes()[0] == ("push", 1, 75, 8, False) and ("push", 1, 7, 8, False) in dev.pushes(), "the 3-frame file goes out padded to 7 frames"
    assert not [n for n in os.listdir(out) if n.endswith(".part")]


def test_streamed_decode_rescale_hold_is_bounded(tmp_path):
    src, out = tmp_path / "tokens", tmp_path / "audio"
    src.mkdir()
    np.save(src / "a_long.npy", _tokens(8, 4 * 75, 1))
    np.save(src / "b_short.npy", _tokens(8, 75, 2))
    tok = _tok(decoder=_StubDecoder())
    tok.decode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=0, token_dir=src, rescale=True, device_writer=False, stream=True,
                           max_held_bytes=4 * HOP * 75 * 2)      # two ticks of one file
    assert [os.path.basename(p) for p, _ in tok.skipped_files] == ["a_long.npy"] and "max_held_bytes" in tok.skipped_files[0][1]
    assert os.listdir(out) == ["b_short.wav"] and len(_read_wav(out / "b_short.wav")) == HOP * 75
