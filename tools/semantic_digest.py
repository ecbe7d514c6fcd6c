#!/usr/bin/env python3
"""One sha256 per output of a fixed, seeded table of semantic_m / semantic_s encode calls: the bit-identity check of a change that must not change
results (a refactor of the host code, a rebuilt toolchain). Run it on two builds on the same machine and diff the listings:

    python tools/semantic_digest.py > a.txt        # AUDIOTOKEN_HIP_LIB selects the library, as everywhere

Both models are 3-layer synthetic ones, B = 3 with ragged masks (full, two thirds, just over the shortest clip). semantic_m: N = 880 (T = 2), 10800
(T = 33) and 48400 (T = 150, two row tiles), each with pad multiple 0 and 4; B = 1, N = 560000 (T = 1749: past the 8-wave attention's T <= 1728, so its
round-3 twin runs) with the defaults only. semantic_s: N = 400 (T = 1), 1200, 10640, 82000 (T = 256, a full row tile) and 96077 (T = 299). Every length
runs with the defaults, arith = bf16x3 and f32, each boolean option of the model off, attn_w8 = 0, layer 1 pinned to bf16x3 under f16x2 (neighbouring
layers differ in scheme; semantic_s also with ln_split = 0) and n_layers = 0, 1, 2. Per call: tokens, hidden states (semantic_m: features and attention
mask too), the status word, and one hash over range_report, layer_status, site_scales and the profiler's groups with their launch counts. Per model: the
packed meta and blob after the default runs, and again after bf16x3 has been split as well. A few seconds in total.
"""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import HubertEncoderConfig, Wav2VecBertConfig  # noqa: E402
from audiotoken_amd.encoder import Wav2VecBertEncoder  # noqa: E402
from audiotoken_amd.hubert import HubertEncoder  # noqa: E402

M_LENGTHS, M_PADS, M_MIN = (880, 10800, 48400), (0, 4), 560
S_LENGTHS, S_MIN = (400, 1200, 10640, 82000, 96077), 400
M_BOOLS = ("dwconv_stream", "vq_split", "vq_refine")
S_BOOLS = ("posconv_split", "ln_split", "kmeans_split", "vq_refine")
PIN = {"layer_arith:1": "bf16x3"}


def configs(bools, with_ln_pin):
    """(name, {option: value}, n_layers or None), in the order they run: defaults first, so that only f16x2 is split when the first export is taken"""
    out = [("defaults", {}, None), ("arith=bf16x3", {"arith": "bf16x3"}, None), ("arith=f32", {"arith": "f32"}, None)]
    out += [(f"{b}=0", {b: 0}, None) for b in bools]
    out += [("attn_w8=0", {"attn_w8": 0}, None), ("layer_arith:1=bf16x3", dict(PIN), None)]
    if with_ln_pin:
        out += [("layer_arith:1=bf16x3 ln_split=0", dict(PIN, ln_split=0), None)]
    return out + [(f"n_layers={n}", {}, n) for n in (0, 1, 2)]


def sha(x) -> str:
    if isinstance(x, torch.Tensor):
        x = x.detach().contiguous().cpu().numpy().tobytes()
    elif not isinstance(x, bytes):
        x = repr(x).encode()
    return hashlib.sha256(x).hexdigest()


class options:
    """the given options set inside the block, restored afterwards"""

    def __init__(self, model, values):
        self.model, self.values = model, values

    def __enter__(self):
        self.saved = {n: self.model.get_option(n) for n in self.values}
        for n, v in self.values.items():
            self.model.set_option(n, v)

    def __exit__(self, *exc):
        for n, v in self.saved.items():
            self.model.set_option(n, v)


def batch(B: int, n: int, shortest: int, seed: int):
    wav = torch.from_numpy(W.synth_waveform(B, n, 16000, seed=seed)).cuda()
    mask = torch.zeros(B, n)
    for b, valid in enumerate((n, max(2 * n // 3, shortest), shortest + 1)[:B]):
        mask[b, :min(valid, n)] = 1.0
    return wav, mask.cuda()


def line(name: str, model, **tensors) -> None:
    status = model.last_status()   # synchronises
    launches = [(k, v[1]) for k, v in model.read_profile().items()]
    reports = (sorted(model.range_report().items()), model.layer_status(), model.site_scales(), launches)
    print(f"{name:62s} status={status} " + " ".join(f"{k}={sha(v)}" for k, v in tensors.items()) + f" reports={sha(reports)}", flush=True)


def export_line(name: str, model) -> None:
    meta, blob = model.export_packed()
    print(f"{name:62s} meta={sha(bytes(meta))} blob={sha(blob)}", flush=True)


def run(tag, model, call, lengths, shortest, bools, with_ln_pin) -> None:
    for cfg, opts, n_layers in configs(bools, with_ln_pin):
        with options(model, opts):
            for n, extra in lengths:
                wav, mask = batch(3, n, shortest, seed=9000 + n)
                model.enable_profile(True)   # (restarts the profiler: the launch counts are this call's)
                line(f"{tag} B=3 N={n}{extra[0]} {cfg}", model, **call(wav, mask, n_layers, *extra[1:]))
        if cfg == "defaults":
            export_line(f"{tag} packed after the default runs", model)
        if cfg == "arith=bf16x3":
            export_line(f"{tag} packed after bf16x3 was split too", model)


def semantic_m() -> None:
    enc = Wav2VecBertEncoder(Wav2VecBertConfig(output_layer=3), device="cuda:0", weights=W.synth_w2vbert_weights(n_layers=3, seed=5, with_vq=True))

    def call(wav, mask, n_layers, pad=2):
        tok, taps = enc(wav, mask, pad_to_multiple_of=pad, n_layers=n_layers, return_taps=True)
        return dict(tokens=tok, hidden=taps["hidden"], features=taps["input_features"], attention_mask=taps["attention_mask"])

    run("semantic_m", enc, call, [(n, (f" pad={p}", p)) for n in M_LENGTHS for p in M_PADS], M_MIN, M_BOOLS, False)
    wav, mask = batch(1, 560000, M_MIN, seed=9999)
    enc.enable_profile(True)
    line("semantic_m B=1 N=560000 pad=2 defaults", enc, **call(wav, mask, None))


def semantic_s() -> None:
    enc = HubertEncoder(HubertEncoderConfig(output_layer=3), device="cuda:0", weights=W.synth_hubert_weights(n_layers=3, with_kmeans=True))

    def call(wav, mask, n_layers):
        tok, hidden = enc(wav, mask, n_layers=n_layers, return_hidden=True)
        return dict(tokens=tok, hidden=hidden)

    run("semantic_s", enc, call, [(n, ("",)) for n in S_LENGTHS], S_MIN, S_BOOLS, True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device"
    semantic_m()
    semantic_s()
