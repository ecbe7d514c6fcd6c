#!/usr/bin/env python
"""The device FLAC encoder against what it follows (recorded in profiles/flac_writer.txt), in one run on one device:

  decode   AcousticDecoder.forward + status read on the decode leg's batch (``--batch`` rows of ``--seconds`` s, tokens on the device), HIP events;
  pcm      at_pcm_pack on that batch's float output;
  flac     at_flac_encode_rows (encode kernel + scan + compaction) on the same float output;
  ratio    bytes of the FLAC files / bytes of the WAV files, every row written as a file of its own, for (a) the synthetic decoder's output, which is
           heavily clipped, and (b) ``weights.synth_waveform`` (amplitude 0.3).

``--decode-only`` times the decode alone and imports nothing the FLAC feature added (to time the commit before it with the same script).
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402

HOP, K, SR = 320, 8, 24000


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def flac_leg(src, batch, n, warmup, reps):
    """(ms per launch, ratio of file bytes FLAC / WAV) of at_flac_encode_rows on ``batch`` rows of ``n`` floats."""
    from audiotoken_amd import _cabi
    from audiotoken_amd import writer as Wr
    lib = _cabi.load()
    dev = src.device
    descs, nblocks = Wr._flac_rows([(b * n, 0, n, 1.0) for b in range(batch)])
    arr = (_cabi.FlacRowDesc * batch)(*[_cabi.FlacRowDesc(*d) for d in descs])
    descs_dev = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)
    cap = nblocks + 2 * batch * n
    recs = torch.empty(40 * nblocks, dtype=torch.uint8, device=dev)
    out = torch.empty(cap, dtype=torch.uint8, device=dev)
    counts = torch.empty((batch, 2), dtype=torch.int32, device=dev)
    ws_bytes = lib.at_flac_encode_workspace_bytes(nblocks)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

    def launch():
        rc = lib.at_flac_encode_rows(src.data_ptr(), descs_dev.data_ptr(), batch, nblocks, 0.99, recs.data_ptr(), out.data_ptr(), cap, counts.data_ptr(), ws.data_ptr(),
                                     ws_bytes, stream)
        assert rc == 0, _cabi.last_error()
    ms = timed(launch, warmup, reps)
    r = recs.cpu().numpy().view(_cabi.FLAC_BLOCK_DTYPE)
    data = out.cpu().numpy()
    flac_bytes = 0
    for b in range(batch):
        frames, _ = Wr.flac_frames(r[r["row"] == b], data, SR, np.zeros(batch, np.int64))
        flac_bytes += 42 + len(frames)
    kinds = {name: int((r["kind"] == v).sum()) for name, v in (("constant", 0), ("verbatim", 1), ("fixed", 2))}
    return ms, flac_bytes / float(batch * (44 + 2 * n)), kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--seconds", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--decode-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a HIP device"
    frames = 75 * a.seconds
    n = HOP * frames
    tok = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=K, weights=W.synth_encodec_weights(seed=0, with_decoder=True))
    tok.load_decoder()
    dec = tok.decoder
    g = torch.Generator().manual_seed(1)
    toks = torch.randint(0, 1024, (a.batch, K, frames), dtype=torch.int64, generator=g).cuda()

    def decode():
        dec(toks)
        dec.last_status()
    res = {"batch": a.batch, "seconds": a.seconds, "reps": a.reps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "decode_ms": round(timed(decode, a.warmup, max(3, a.reps // 4)), 4)}
    if not a.decode_only:
        from audiotoken_amd import writer as Wr
        wav = dec.forward(toks).reshape(-1).contiguous()
        assert dec.last_status() == 0 and wav.numel() == a.batch * n
        wr = Wr.DeviceWriter("cuda:0")
        descs = wr._descs([(b * n, b * n, n, 1.0) for b in range(a.batch)], wav.numel())
        dst = torch.empty(a.batch * n, dtype=torch.int16, device="cuda:0")
        counts = torch.empty((a.batch, 2), dtype=torch.int32, device="cuda:0")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        res["pcm_pack_ms"] = round(timed(lambda: wr.lib.at_pcm_pack(wav.data_ptr(), descs.data_ptr(), a.batch, n, 0.99, dst.data_ptr(), counts.data_ptr(), stream),
                                         a.warmup, a.reps), 4)
        ms, ratio, kinds = flac_leg(wav, a.batch, n, a.warmup, a.reps)
        res["flac_encode_ms"], res["ratio_decoder_output"], res["blocks_decoder_output"] = round(ms, 4), round(ratio, 4), kinds
        res["clipped_fraction_decoder_output"] = round(float((wav.abs() > 0.99).float().mean()), 4)
        synth = torch.from_numpy(W.synth_waveform(a.batch, n, SR, seed=77)).cuda().reshape(-1).contiguous()
        ms, ratio, kinds = flac_leg(synth, a.batch, n, a.warmup, a.reps)
        res["flac_encode_ms_synth_waveform"], res["ratio_synth_waveform"], res["blocks_synth_waveform"] = round(ms, 4), round(ratio, 4), kinds
        res["flac_over_decode"] = round(res["flac_encode_ms"] / res["decode_ms"], 4)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
