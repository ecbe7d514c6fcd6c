#!/usr/bin/env python3
"""One sha256 per output of a fixed, seeded table of acoustic encode / decode calls: the bit-identity check of a change that must not change results
(a refactor of the host code, a rebuilt toolchain). Run it on two builds on the same machine and diff the listings:

    python tools/acoustic_digest.py > a.txt        # AUDIOTOKEN_HIP_LIB selects the library, as everywhere

Encode (ids, embeddings, status word): B = 3 at four lengths of tests/acoustic_routes.py (all-unfused short clip, stand-alone split route, and the
fully fused stack with ragged tiles, odd and even) with the defaults and with each option group that selects other kernels switched off; B = 81 with
subbatch 2; a 3-push stream with its state. Decode (waveform, status): B = 2 at T = 7 and 75 with the defaults and each decoder option off; a 3-push stream.
A few seconds in total.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import AcousticDecoderConfig, AcousticEncoderConfig  # noqa: E402
from audiotoken_amd.decoder import AcousticDecoder  # noqa: E402
from audiotoken_amd.encoder import AcousticEncoder  # noqa: E402

ENC_LENGTHS = (321, 2202, 14400, 22719)
FUSED = ("fused_stage0", "fused_res64", "fused_res128", "fused_down64", "fused_stage1")
ENC_CONFIGS = (("defaults", ()), ("res_f16x2=0", ("res_f16x2",)), ("chain_f16x2=0", ("chain_f16x2",)), ("lstm_pipe=0", ("lstm_pipe",)),
               ("lstm_f16x2=0", ("lstm_f16x2",)), ("persistent_lstm=0", ("persistent_lstm",)), ("fused=0", FUSED))
DEC_FRAMES = (7, 75)
DEC_CONFIGS = (("defaults", ()), ("dec_chain=0", ("dec_chain",)), ("up_f16x2=0", ("up_f16x2",)), ("fused_dectail=0", ("fused_dectail",)))


def sha(t: torch.Tensor) -> str:
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def line(name: str, model, **tensors) -> None:
    status = model.last_status()   # synchronises
    print(f"{name:46s} status={status} " + " ".join(f"{k}={sha(v)}" for k, v in tensors.items()), flush=True)


class switched_off:
    """the named boolean options at 0 inside the block, restored afterwards"""

    def __init__(self, model, names):
        self.model, self.names = model, names

    def __enter__(self):
        self.saved = {n: self.model.get_option(n) for n in self.names}
        for n in self.names:
            self.model.set_option(n, 0)

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            self.model.set_option(n, v)


def tokens(B: int, K: int, T: int, seed: int) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).integers(0, W.ENCODEC_CODEBOOK, size=(B, K, T), dtype=np.int64))


def encode_side() -> None:
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    for cfg, off in ENC_CONFIGS:
        with switched_off(enc, off):
            for n in ENC_LENGTHS:
                wav = torch.from_numpy(W.synth_waveform(3, n, 24000, seed=7000 + n)).cuda()
                ids, emb = enc(wav, return_embeddings=True)
                line(f"encode B=3 N={n} {cfg}", enc, ids=ids, emb=emb)
    saved = enc.get_option("subbatch")
    enc.set_option("subbatch", 2)
    wav = torch.from_numpy(W.synth_waveform(81, 633, 24000, seed=7633)).cuda()
    ids, emb = enc(wav, return_embeddings=True)
    line("encode B=81 N=633 subbatch=2", enc, ids=ids, emb=emb)
    enc.set_option("subbatch", saved)
    # a stream of 2240 + 3200 + (final) 1000 samples, straight through the library's push, past the residual buffering. The two seams are those of
    # streaming._Stream, which both lockstep streams are: _device_push(x, final) is one transaction (the bare push, the ladder, the swap) and _state
    # its pair of state buffers, so after a push _state[0] is what it wrote and _state[1] what it read. decode_side() uses the same two.
    st = enc.new_stream(batch=3)
    st._state[1].zero_()
    wav = torch.from_numpy(W.synth_waveform(3, 6440, 24000, seed=7999)).cuda()
    at = 0
    for i, (n, final) in enumerate(((2240, False), (3200, False), (1000, True))):
        ids = st._device_push(wav[:, at:at + n].contiguous(), final)
        at += n
        line(f"encode stream push {i} n={n} final={int(final)}", enc, ids=ids, state=st._state[0], other_state=st._state[1])


def decode_side() -> None:
    dec = AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=True))
    for cfg, off in DEC_CONFIGS:
        with switched_off(dec, off):
            for T in DEC_FRAMES:
                line(f"decode B=2 T={T} {cfg}", dec, wav=dec(tokens(2, 8, T, 8000 + T)))
    st = dec.new_stream(batch=2)
    st._state[1].zero_()
    tok = tokens(2, 8, 15, 8999).cuda()
    at = 0
    for i, t in enumerate((7, 5, 3)):
        wav = st._device_push(tok[:, :, at:at + t].contiguous())
        at += t
        line(f"decode stream push {i} t={t}", dec, wav=wav, state=st._state[0])


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device"
    encode_side()
    decode_side()
