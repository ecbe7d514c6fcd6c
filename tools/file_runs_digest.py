#!/usr/bin/env python3
"""What a fixed, seeded table of whole-file runs leaves behind (``encode_batch_files``, ``decode_batch_files``, ``fit_quantizer``): the check of a change to
the Python drivers that must not change results. Run it on two checkouts on the same machine and diff the listings:

    python tools/file_runs_digest.py --cpu > a.txt        # stand-in models, no device
    python tools/file_runs_digest.py --gpu > b.txt        # the real models with synthetic weights (AUDIOTOKEN_HIP_LIB selects the library, as everywhere)

Per case: one line per output file (relative path, sha256 of its bytes), the ``skipped_files`` entries (basename, reason), ``run_summary`` with sorted keys,
the batches / rows counters and the NAMES of the timing keys (no wall-clock value is printed), an exception that ended the run, and in ``--cpu`` mode the
stand-ins' call logs (the stub decoder's (B, K, T) list, the stream pool's pushes). Every run is in a temporary directory, whose path is printed as <tmp>.

Encode corpus (24 kHz int16 WAV): 400, 12000, 24000, 24002 samples, 2.7 s and 3.3 s, in a small tree; a stereo file, a 300-sample file, a garbage
``.wav`` and an empty ``.tar``. Decode corpus: token files of T = 3, 75, 80, 159 and 375 frames with K = 2 and 8, one int16 and one ``[1, K, T]``.
``--cpu``: the stand-ins of the CPU tests (tests/test_distributed_cpu.py, test_stream_files_cpu.py, test_decode_files_cpu.py). ``--gpu`` adds
``resample="file"`` on a 16 kHz and a 44.1 kHz file, one semantic_m and one semantic_s run, the device writer, and one ``fit_quantizer`` call (run twice:
the centres' hash is printed only if the two runs agree). Seconds in total.
"""
import argparse
import hashlib
import os
import sys
import tempfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402

SR, HOP = 24000, 320
ENC_FILES = {"a.wav": 12000, "b.wav": 24000, "sub/c.wav": 24002, "sub/deep/d.wav": int(2.7 * SR), "sub/deep/e.wav": int(3.3 * SR), "f.wav": 400}
DEC_FILES = {"a.npy": (8, 159), "b.npy": (8, 3), "c.npy": (2, 80), "d.npy": (8, 75), "deep/e.npy": (8, 375)}
TMP = ""


def clean(text) -> str:
    return str(text).replace(TMP, "<tmp>")


def listing(root) -> None:
    found = sorted(os.path.relpath(os.path.join(d, n), root) for d, _, names in os.walk(root) for n in names) if os.path.isdir(root) else []
    for rel in found:
        with open(os.path.join(root, rel), "rb") as fh:
            print(f"  file {rel} {hashlib.sha256(fh.read()).hexdigest()}")
    if not found:
        print("  no output file")


def report(name: str, tok, out, call, logs=()) -> None:
    """Run ``call`` and print what it left: on ``tok`` and under ``out``."""
    print(f"== {name}", flush=True)
    tok.skipped_files, tok.run_summary, tok.run_timings = [], {}, {}
    try:
        call()
    except Exception as e:   # noqa: BLE001 — a run that ends in an exception is a case of the table: what it left behind is listed all the same
        print(f"  raised {type(e).__name__}: {clean(e)}")
    listing(out)
    for path, why in tok.skipped_files:
        print(f"  skipped {os.path.basename(str(path))}: {clean(why)}")
    print("  run_summary " + " ".join(f"{k}={tok.run_summary[k]}" for k in sorted(tok.run_summary)))
    rt = tok.run_timings
    print(f"  batches={rt.get('batches')} rows={rt.get('rows')} timing keys: {' '.join(sorted(rt))}")
    for label, log in logs:
        print(f"  {label} {log()}")
    sys.stdout.flush()


# ---- corpora ----------------------------------------------------------------------------------------------------------------------------------------------------
def write_wav(path, x, sr) -> None:
    from scipy.io import wavfile
    os.makedirs(os.path.dirname(path), exist_ok=True)
    wavfile.write(path, sr, np.round(np.asarray(x) * 20000).astype(np.int16))


def encode_corpus(root) -> None:
    for i, (name, n) in enumerate(sorted(ENC_FILES.items())):
        write_wav(os.path.join(root, name), W.synth_waveform(1, n, SR, seed=700 + i)[0], SR)
    write_wav(os.path.join(root, "bad_stereo.wav"), np.zeros((SR, 2)), SR)
    write_wav(os.path.join(root, "tiny.wav"), W.synth_waveform(1, 300, SR, seed=720)[0], SR)
    with open(os.path.join(root, "garbage.wav"), "wb") as fh:
        fh.write(b"RIFF\x00\x00 not a wave file")
    with open(os.path.join(root, "zz_members.tar"), "wb"):
        pass


def encode_list(root):
    """The corpus as a file list: not in sorted order, the archive last."""
    names = ["sub/deep/e.wav", "a.wav", "garbage.wav", "sub/c.wav", "bad_stereo.wav", "b.wav", "tiny.wav", "f.wav", "sub/deep/d.wav", "zz_members.tar"]
    return [os.path.join(root, n) for n in names]


def decode_corpus(root) -> None:
    for i, (name, (K, T)) in enumerate(sorted(DEC_FILES.items())):
        t = np.random.default_rng(40 + i).integers(0, 1024, size=(K, T)).astype(np.int64)
        os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
        np.save(os.path.join(root, name), t.astype(np.int16) if name == "a.npy" else (t[None] if name == "d.npy" else t))


# ---- the tables --------------------------------------------------------------------------------------------------------------------------------------------------
def encode_cases(make_tok, chunked_options, logs_of=lambda tok: ()) -> None:
    """``make_tok(stream)`` -> a fresh AudioToken; ``chunked_options``: [(label, keyword arguments)] of the chunked runs."""
    src = os.path.join(TMP, "audio")
    encode_corpus(src)
    n = 0
    for where in ("audio_dir", "audio_files"):
        inputs = {"audio_dir": src} if where == "audio_dir" else {"audio_files": encode_list(src)}
        for label, kw in chunked_options:
            tok, out = make_tok(False), os.path.join(TMP, f"tokens{n}")
            n += 1
            report(f"encode chunked {where} {label}", tok, out,
                   lambda: tok.encode_batch_files(batch_size=3, outdir=out, chunk_size=1, **inputs, **kw), logs_of(tok))
        if where == "audio_files":     # the empty archive ends the runs above with tarfile's exception: once without it, so that a run also ends well
            tok, out, (label, kw) = make_tok(False), os.path.join(TMP, f"tokens{n}"), chunked_options[-1]
            n += 1
            report(f"encode chunked audio_files without the archive {label}", tok, out,
                   lambda: tok.encode_batch_files(batch_size=3, outdir=out, chunk_size=1, audio_files=inputs["audio_files"][:-1], **kw), logs_of(tok))
        tok, out = make_tok(True), os.path.join(TMP, f"tokens{n}")
        n += 1
        report(f"encode stream {where}", tok, out,
               lambda: tok.encode_batch_files(batch_size=3, outdir=out, chunk_size=1, num_workers=2 if where == "audio_dir" else 0, stream=True, **inputs),
               logs_of(tok))


def decode_cases(make_tok, device_writers=(False,), logs_of=lambda tok: (), failing=None) -> None:
    src = os.path.join(TMP, "tokens_in")
    decode_corpus(src)
    n = 0

    def run(name, tok, **kw):
        nonlocal n
        out = os.path.join(TMP, f"audio_out{n}")
        n += 1
        kw.setdefault("token_dir", src)
        report(name, tok, out, lambda: tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=1, **kw), logs_of(tok))

    for dw in device_writers:
        for fmt in ("wav", "flac"):
            for rescale in (False, True):
                for stream in (False, True):
                    run(f"decode {fmt} rescale={rescale} stream={stream} device_writer={dw}", make_tok(), num_workers=2, rescale=rescale, audio_format=fmt,
                        stream=stream, device_writer=dw)
    dw = device_writers[0]
    os.makedirs(os.path.join(src, "twin"), exist_ok=True)
    np.save(os.path.join(src, "twin", "a.npy"), np.random.default_rng(50).integers(0, 1024, size=(8, 20)).astype(np.int64))
    with open(os.path.join(src, "z_bad.npy"), "wb") as fh:
        fh.write(b"\x93NUMPY\x01\x00 this header never ends")
    run("decode a duplicate output name and an invalid token file", make_tok(), num_workers=0, device_writer=dw, token_dir=None,
        token_files=[os.path.join(src, x) for x in ("a.npy", "z_bad.npy", "twin/a.npy", "c.npy")])
    os.remove(os.path.join(src, "z_bad.npy"))
    os.remove(os.path.join(src, "twin", "a.npy"))
    if failing is not None:
        run("decode, the third decoder call fails", failing(), num_workers=0, device_writer=dw)
    for stream in (False, True):
        run(f"decode rescale max_held_bytes drops a file stream={stream}", make_tok(), num_workers=0, rescale=True, stream=stream, device_writer=dw,
            max_held_bytes=4 * HOP * 75 * 2)


# ---- --cpu -------------------------------------------------------------------------------------------------------------------------------------------------------
def cpu_table() -> None:
    from audiotoken_amd.streaming import AcousticDecodeStreamPool
    from tests.test_decode_files_cpu import _StubDecoder
    from tests.test_distributed_cpu import _HashEncoder
    from tests.test_stream_files_cpu import _StubEncoder
    from tests.test_stream_pool_cpu import StubDevice

    class Decoder(_StubDecoder):
        """The chunked stand-in with the stream pool of tests/test_stream_files_cpu.py's."""

        def __init__(self, fail_at=None):
            super().__init__(fail_at)
            self.devices = []

        def new_stream_pool(self, slots):
            dev = StubDevice(slots)

            def push(toks, started):
                dev.push_decode(toks, started)
                return self.forward(toks).reshape(toks.shape[0], -1)
            self.devices.append(dev)
            return AcousticDecodeStreamPool(None, slots, push_fn=push, gather_fn=dev.gather, scatter_fn=dev.scatter)

    def enc_tok(stream):
        tok = AudioToken(Tokenizers.acoustic, device="cpu", num_codebooks=8 if stream else 2)
        tok.encoder = _StubEncoder() if stream else _HashEncoder()
        return tok

    def dec_tok(fail_at=None):
        tok = AudioToken(Tokenizers.acoustic, device="cpu", num_codebooks=8)
        tok.decoder = Decoder(fail_at)
        return tok

    def pushes(model):
        return lambda: [e for d in model.devices for e in d.pushes()]

    encode_cases(enc_tok, [("num_workers=0", dict(num_workers=0, device_feeder=False)), ("num_workers=2", dict(num_workers=2, device_feeder=False)),
                           ("worker_processes", dict(num_workers=2, device_feeder=False, worker_processes=True))],
                 lambda tok: [("pool pushes", pushes(tok.encoder))] if hasattr(tok.encoder, "devices") else [])
    decode_cases(dec_tok, logs_of=lambda tok: [("decoder calls", lambda: tok.decoder.calls), ("pool pushes", pushes(tok.decoder))],
                 failing=lambda: dec_tok(fail_at=3))


# ---- --gpu -------------------------------------------------------------------------------------------------------------------------------------------------------
def gpu_table() -> None:
    assert torch.cuda.is_available(), "needs a HIP device"
    from audiotoken_amd.synthetic import speech_like_waveform
    w = W.synth_encodec_weights(seed=0, with_decoder=True)
    one = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=8, weights=w)      # (one model for all acoustic cases: `report` clears what a run left)
    acoustic = lambda *_: one
    encode_cases(acoustic, [("num_workers=0", dict(num_workers=0)), ("num_workers=2", dict(num_workers=2))])

    src = os.path.join(TMP, "rates")
    for i, sr in enumerate((16000, 44100)):
        write_wav(os.path.join(src, f"r{sr}.wav"), W.synth_waveform(1, int(2.3 * sr) + 17, sr, seed=730 + i)[0], sr)
    tok, out = acoustic(), os.path.join(TMP, "tokens_rates")
    report('encode stream resample="file" 16 kHz and 44.1 kHz', tok, out,
           lambda: tok.encode_batch_files(batch_size=2, outdir=out, chunk_size=1, num_workers=0, audio_dir=src, stream=True, resample="file"))

    src = os.path.join(TMP, "speech")
    x = speech_like_waveform(3, 7 * 16000, 16000, seed=77)
    for i in range(3):
        write_wav(os.path.join(src, f"clip{i}.wav"), x[i] / max(1.0, float(np.abs(x[i]).max())), 16000)
    sem_w = {"semantic_m": W.synth_w2vbert_weights(n_layers=3, seed=5, with_vq=True), "semantic_s": W.synth_hubert_weights(n_layers=3, with_kmeans=True)}
    for which in ("semantic_m", "semantic_s"):
        tok, out = AudioToken(Tokenizers(which), device="cuda:0", weights=sem_w[which]), os.path.join(TMP, f"tokens_{which}")
        tok.model_config.output_layer = 3
        report(f"encode chunked {which}, three files in 2 s chunks", tok, out,
               lambda: tok.encode_batch_files(batch_size=4, outdir=out, chunk_size=2, num_workers=0, audio_dir=src))

    decode_cases(acoustic, device_writers=(True, False))

    # 3 x 7 s at 50 frames a second = 1050 frames for the 1000 codes of semantic_s: the smallest corpus of whole seconds that can be fitted
    fits = []
    for i in range(2):
        tok = AudioToken(Tokenizers.semantic_s, device="cuda:0", weights=W.synth_hubert_weights(3, 6, False))
        tok.model_config.output_layer = 3
        fits.append(tok.fit_quantizer(os.path.join(TMP, f"km{i}.bin"), audio_dir=src, chunk_size=30, batch_size=2, num_workers=0, max_frames=2000, max_iter=3,
                                      seed=0))
    print("== fit_quantizer semantic_s")
    print("  fit_summary_ " + " ".join(f"{k}={fits[0].fit_summary_[k]}" for k in sorted(fits[0].fit_summary_)))
    a, b = (np.ascontiguousarray(f.cluster_centers_) for f in fits)
    if a.tobytes() == b.tobytes():
        print(f"  centres {hashlib.sha256(a.tobytes()).hexdigest()} (two runs agree)")
    else:
        print("  centres differ between two runs of one build: fit_summary_ only")


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    mode = ap.add_mutually_exclusive_group(required=True)
    mode.add_argument("--cpu", action="store_true")
    mode.add_argument("--gpu", action="store_true")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        TMP = os.path.realpath(tmp)
        (cpu_table if args.cpu else gpu_table)()
