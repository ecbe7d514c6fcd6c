#!/usr/bin/env python3
"""The fine stage with a history prompt (csrc/fine.hip): what a history costs, and that the call without one costs what it did (writes
profiles/fine_history.txt).

    python tools/fine_history_bench.py [--out-dir profiles] [--reps 3] [--tag this]

Needs the MI355X. §18's 12-layer / 768 synthetic model at W = 1024 (H = 512), temperature 0.5, B rows of T frames in one lockstep ``generate`` call; every
figure is device-event time around the call with its closing copy, one warm-up, then the median of --reps calls with the min .. max spread, the protocol of
profiles/long_form.txt. Legs, at B = 1 and 16:

  T = 2048 without a history          3 windows, rel = 0 in each: the head runs on all 1024 rows of a window
  T = 2048 after a 600-frame history  h = 512 cells in front: 4 windows, rel = 512 in each: one more window, the head on 512 rows of each
  T = 512 without / with the history  one window each; with the history the head runs on half of it, everything else is the same work

The file also runs under a checkout whose ``generate`` has no ``history=``: it then times the legs without a history only, which is how the parent commit's
build is measured for the comparison (--tag names the build in the output).
"""
import argparse
import inspect
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--tag", default="this build")
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.fine_decoder import CoarseToFine, fine_windows, seeded_uniforms  # noqa: E402

BLOCK, TH = 1024, 600
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("fine_history_bench needs the GPU: there is nothing to measure on a CPU")
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    with_history = "history" in inspect.signature(CoarseToFine.generate).parameters
    say(f"tools/fine_history_bench.py on {torch.cuda.get_device_name(0)}, {args.tag}: 12 layers / 768, W = {BLOCK}, temperature 0.5, device-event ms around one "
        f"lockstep generate call with its closing copy, one warm-up, median of {args.reps} [min .. max]")
    dec = CoarseToFine(device="cuda:0", weights=W.synth_fine_weights(12, 768, BLOCK, seed=0, family="uniform"))
    rng = np.random.default_rng(11)
    history = rng.integers(0, 1024, size=(8, TH))
    for B in (1, 16):
        for T in (2048, 512):
            rows = [rng.integers(0, 1024, size=(2, T)) for _ in range(B)]
            legs = [("no history", None, 0)] + ([(f"{TH}-frame history", history, BLOCK // 2)] if with_history else [])
            for name, hist, h in legs:
                n = len(fine_windows(T, BLOCK, h)) if h else len(fine_windows(T, BLOCK))
                u = seeded_uniforms(5, B, n, BLOCK)
                kw = {"history": hist} if hist is not None else {}
                call = lambda: dec.generate(rows, temperature=0.5, uniforms=u, **kw)
                call()
                ms = [once(call) for _ in range(args.reps)]
                med = statistics.median(ms)
                say(f"  B = {B:2d}, T = {T:4d}, {name:18s}: {n} windows, {med:9.2f} ms [{min(ms):.2f} .. {max(ms):.2f}], {med / n:8.2f} ms a window, "
                    f"{B * T / med * 1e3:10,.0f} frames/s")
    os.makedirs(out_dir, exist_ok=True)
    name = "fine_history.txt" if with_history else "fine_history_parent.txt"
    with open(os.path.join(out_dir, name), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/{name}")


if __name__ == "__main__":
    main()
