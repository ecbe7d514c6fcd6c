#!/usr/bin/env python3
"""Token files -> WAV files: what decode_batch_files delivers, against the device-resident decode and against a loop over the older API
(writes profiles/decode_files.json).

    python tools/decode_files_bench.py [--out profiles/decode_files.json] [--files 256] [--seconds 10] [--batch 64] [--reps 3] [--baseline-only]

Needs the MI355X (no CPU path: without a device it fails). Synthetic weights and seeded random tokens (K = 8); the token files and every output live on
/dev/shm, so no disk is in the measurement. Legs, all over the same ``--files`` files of ``--seconds`` s each, alternating within one run (boxes differ by a
few percent: only ratios within a run mean anything):
  a  ``decode_batch_files(batch_size=--batch, chunk_size=--seconds)``: WALL seconds from the call to its return (every file closed), audio-s / s;
  b  the device-resident decode of the same batches: ``AcousticDecoder.forward`` + status read on tokens that are already on the device, HIP events;
  c  the baseline, built ONLY from the API the commit before this feature has (``--baseline-only`` runs nothing else, on either commit):
     ``AudioToken.decode`` per segment, numpy clamp / scale / round / int16, stdlib ``wave``; WALL seconds;
  c64 the same loop with 64 segments per ``AudioToken.decode`` call (the best a user could do by hand with equal-length segments); WALL seconds;
  d  the pack kernel alone on one batch: HIP events around ``--pack-reps`` launches, bytes = 4 B read + 2 B written per sample, against the measured HBM
     copy roof of MI355X_MICROARCH (6.29 TB/s).
"""
import argparse
import json
import os
import shutil
import statistics
import sys
import time
import wave

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=None)
ap.add_argument("--files", type=int, default=256)
ap.add_argument("--seconds", type=int, default=10)
ap.add_argument("--batch", type=int, default=64)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--pack-reps", type=int, default=50)
ap.add_argument("--workers", type=int, default=12)
ap.add_argument("--baseline-only", action="store_true", help="leg c only (it uses nothing this feature added), one JSON line")
ap.add_argument("--scratch", default="/dev/shm/audiotoken_decode_files_bench")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402

HOP, K, SR = 320, 8, 24000
HBM_ROOF = 6.29e12     # bytes / s, float4 copy (MI355X_MICROARCH)


def make_corpus(root, n_files, frames):
    os.makedirs(root, exist_ok=True)
    g = torch.Generator().manual_seed(1)
    paths = []
    for i in range(n_files):
        p = os.path.join(root, f"f{i:05d}.npy")
        np.save(p, torch.randint(0, 1024, (K, frames), dtype=torch.int64, generator=g).numpy().astype(np.int16))
        paths.append(p)
    return paths


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def baseline_leg(tok, paths, outdir, per_call):
    """Only what the commit before this feature offers: AudioToken.decode, numpy, wave."""
    os.makedirs(outdir, exist_ok=True)
    for i in range(0, len(paths), per_call):
        group = paths[i:i + per_call]
        toks = torch.from_numpy(np.stack([np.load(p) for p in group]).astype(np.int64))
        wav = tok.decode(toks).numpy().reshape(len(group), -1)
        q = np.rint(np.clip(wav, -0.99, 0.99) * np.float32(32768.0)).astype(np.int16)
        for p, row in zip(group, q):
            with wave.open(os.path.join(outdir, os.path.splitext(os.path.basename(p))[0] + ".wav"), "wb") as f:
                f.setnchannels(1); f.setsampwidth(2); f.setframerate(SR)
                f.writeframes(row.tobytes())


def device_leg(tok, paths, batch):
    """Milliseconds of the decode alone, by HIP events: the same batches, tokens already on the device."""
    dec = tok.decoder
    batches = [torch.from_numpy(np.stack([np.load(p) for p in paths[i:i + batch]]).astype(np.int64)).cuda() for i in range(0, len(paths), batch)]
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for t in batches:
        dec(t)
        dec.last_status()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def pack_leg(tok, batch, frames, reps):
    from audiotoken_amd import writer as Wr
    wr = Wr.DeviceWriter("cuda:0")
    n = HOP * frames
    src = (torch.randn(batch * n, device="cuda:0") * 1.5)
    rows = [(b * n, b * n, n, 1.0) for b in range(batch)]
    descs = wr._descs(rows, src.numel())
    dst = torch.empty(batch * n, dtype=torch.int16, device="cuda:0")
    counts = torch.empty((batch, 2), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def launch():
        rc = wr.lib.at_pcm_pack(src.data_ptr(), descs.data_ptr(), batch, n, 0.99, dst.data_ptr(), counts.data_ptr(), stream)
        assert rc == 0
    for _ in range(5):
        launch()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        launch()
    b.record()
    b.synchronize()
    ms = a.elapsed_time(b) / reps
    return ms, 6.0 * batch * n / (ms * 1e-3)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("decode_files_bench needs the GPU: there is nothing to measure on a CPU")
    frames = args.seconds * 75
    audio_s = args.files * args.seconds
    shutil.rmtree(args.scratch, ignore_errors=True)
    try:
        paths = make_corpus(os.path.join(args.scratch, "tokens"), args.files, frames)
        tok = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=K, weights=W.synth_encodec_weights(seed=0, with_decoder=True))
        tok.load_decoder()
        c_out = os.path.join(args.scratch, "c")
        if args.baseline_only:
            baseline_leg(tok, paths, c_out, 1)
            t = [wall(lambda: baseline_leg(tok, paths, c_out, 1)) for _ in range(args.reps)]
            print(json.dumps({"baseline_only": True, "c_wall_s": t, "c_audio_s_per_s": audio_s / statistics.median(t)}))
            return
        a_out, c64_out = os.path.join(args.scratch, "a"), os.path.join(args.scratch, "c64")

        def leg_a():
            tok.decode_batch_files(batch_size=args.batch, outdir=a_out, chunk_size=args.seconds, num_workers=args.workers, token_files=paths)
        leg_c = lambda: baseline_leg(tok, paths, c_out, 1)            # noqa: E731
        leg_c64 = lambda: baseline_leg(tok, paths, c64_out, 64)       # noqa: E731
        for fn in (leg_a, leg_c, leg_c64):      # warm-up: code objects, pinned pool, workspaces, page cache
            fn()
        device_leg(tok, paths, args.batch)
        same = all(open(os.path.join(a_out, n), "rb").read() == open(os.path.join(c64_out, n), "rb").read() for n in sorted(os.listdir(a_out))[:8])
        ta, tb, tc, tc64, stages = [], [], [], [], []
        for _ in range(args.reps):
            ta.append(wall(leg_a))
            stages.append(dict(tok.run_timings))
            tb.append(device_leg(tok, paths, args.batch) * 1e-3)
            tc.append(wall(leg_c))
            tc64.append(wall(leg_c64))
        pack_ms, pack_bps = pack_leg(tok, args.batch, frames, args.pack_reps)
        med = statistics.median
        res = {
            "tool": "tools/decode_files_bench.py", "device": torch.cuda.get_device_name(0),
            "workload": {"files": args.files, "seconds_per_file": args.seconds, "batch": args.batch, "K": K, "audio_s": audio_s, "reps": args.reps,
                         "where": "/dev/shm", "weights": "synthetic seed 0"},
            "a_decode_batch_files": {"wall_s": ta, "audio_s_per_s": audio_s / med(ta), "stage_seconds_of_the_median_like_run": stages[len(stages) // 2],
                                     "summary": tok.run_summary},
            "b_device_resident_decode": {"event_s": tb, "audio_s_per_s": audio_s / med(tb)},
            "c_baseline_decode_per_segment_numpy_wave": {"wall_s": tc, "audio_s_per_s": audio_s / med(tc)},
            "c64_baseline_64_segments_per_call": {"wall_s": tc64, "audio_s_per_s": audio_s / med(tc64)},
            "d_pack_kernel": {"rows": args.batch, "samples_per_row": HOP * frames, "ms": pack_ms, "bytes_per_s": pack_bps, "share_of_hbm_copy_roof": pack_bps / HBM_ROOF,
                              "roof_bytes_per_s": HBM_ROOF},
            "ratios": {"a_over_b": med(tb) / med(ta), "a_over_c": med(tc) / med(ta), "a_over_c64": med(tc64) / med(ta)},
            "a_and_c64_write_the_same_bytes": same,
            "note": "ratios are of audio-s / s (higher is better for a): a_over_b = share of the device-resident decode rate that reaches the files, "
                    "a_over_c = speed-up over the per-segment loop of the older API",
        }
        out = args.out or os.path.join(ROOT, "profiles", "decode_files.json")
        os.makedirs(os.path.dirname(out), exist_ok=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps(res["ratios"]), flush=True)
        print(f"wrote {out}")
    finally:
        shutil.rmtree(args.scratch, ignore_errors=True)


if __name__ == "__main__":
    main()
