#!/usr/bin/env python3
"""The sampler's truncation (csrc/gpt_model.hip: gpt_sample_kernel<true>): what top_p costs a generation step (writes profiles/nucleus.txt).

    python tools/nucleus_bench.py [--out-dir profiles] [--parent-lib PATH] [--prompt 251] [--steps 128] [--reps 3]

Needs the MI355X (no CPU path: without a device it fails). The full-size model (12 layers, 53376 ids, block 1024) on seeded synthetic weights, driven
through the C ABI (at_gpt_generate) so that a library built from the parent commit (--parent-lib, which lacks the new symbols) can run beside this one in
the same process, on the same weights, prompts and draws. Every figure is device-event time around one call, one warm-up, the median of --reps with the
min .. max spread; the time of one step is the difference between a call of 16 + --steps tokens and a call of 16 tokens, divided by --steps, the
configurations taking turns inside every repetition. At B = 1, 16 and 64:

  parent           the parent commit's library, when given
  off              this library, truncation off: the same launches as the parent's
  top_p 0.9        top_k = 100: the top-k set is compacted into LDS and the nucleus found there (one more walk over the row)
  top_p 0.9, k=V   top_k = V: the radix descent on masses (four more walks over the row)

and the sampler alone (at_op_topk_sample / at_op_nucleus_sample on 53376 random logits per row) the same way. The added microseconds per step stand next
to what the extra walks over V floats per row would cost one workgroup reading them from L2 at 64 bytes per clock (2.4 GHz)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ap = argparse.ArgumentParser()
ap.add_argument("--out-dir", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--prompt", type=int, default=251)
ap.add_argument("--steps", type=int, default=128)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from audiotoken_amd import _cabi  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.semantic_decoder import seeded_uniforms  # noqa: E402

DEV = torch.device("cuda", 0)
BASE = 16
L2_BYTES_PER_S = 64 * 2.4e9   # one CU's path to L2
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


class Gpt:
    """One library's GPT handle through the C ABI alone; ``path`` None: this package's library."""

    NAMES = ("at_gpt_create", "at_gpt_set_tensor", "at_gpt_finalize", "at_gpt_destroy", "at_gpt_state_bytes", "at_gpt_generate", "at_op_topk_sample")

    def __init__(self, path, tensors):
        if path is None:
            self.lib = _cabi.load()
        else:
            self.lib = C.CDLL(path)
            for name in self.NAMES:
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = _cabi.SIGNATURES[name]
        self.h = self.lib.at_gpt_create(0)
        assert self.h, "at_gpt_create failed"
        for name, arr in tensors.items():
            _cabi.set_tensor(self.lib, self.lib.at_gpt_set_tensor, self.h, name, arr)
        assert self.lib.at_gpt_finalize(self.h) == 0, "at_gpt_finalize failed"
        self.state = None

    def generate(self, d_prompts, lens, n_new, d_u, top_k, out):
        B, stride = d_prompts.shape
        max_len = min(1024, stride + n_new)
        nbytes = self.lib.at_gpt_state_bytes(self.h, B, max_len)
        if self.state is None or self.state.numel() < nbytes:
            self.state = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        u = d_u[:, :n_new].contiguous()
        rc = self.lib.at_gpt_generate(self.h, d_prompts.data_ptr(), stride, (C.c_int32 * B)(*lens), B, n_new, 0.8, top_k, -1, u.data_ptr(), None, out[0].data_ptr(),
                                      out[1].data_ptr(), out[2].data_ptr(), None, self.state.data_ptr(), self.state.numel(), max_len,
                                      _cabi.current_stream_handle(DEV), None)
        assert rc == 0, "at_gpt_generate failed"


def measure(configs, reps):
    """{name: [per-repetition value]}: ``configs`` is {name: thunk returning one value}; the thunks take turns inside every repetition, after one warm-up."""
    for fn in configs.values():
        fn()
    out = {name: [] for name in configs}
    for _ in range(reps):
        for name, fn in configs.items():
            out[name].append(fn())
    return out


def line(name, xs, unit, ref=None):
    med = statistics.median(xs)
    tail = "" if ref is None else f"; {med - ref:+.2f} {unit} against the parent ({med / ref:.3f} x)"
    return med, f"  {name:<16} {med:9.2f} {unit} [{min(xs):.2f} .. {max(xs):.2f}]{tail}"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("nucleus_bench needs the GPU: there is nothing to measure on a CPU")
    cfg = Wav2VecBertDecoderConfig()
    V = cfg.VOCAB_SIZE
    out_dir = args.out_dir or os.path.join(ROOT, "profiles")
    tensors = W.gpt_tensors_from_state_dict(W.synth_gpt_weights(n_layer=12, vocab=V, block=1024, seed=0, family="uniform"), "weights dict")
    new = Gpt(None, tensors)
    parent = Gpt(args.parent_lib, tensors) if args.parent_lib else None
    walk_us = V * 4 / L2_BYTES_PER_S * 1e6
    say(f"tools/nucleus_bench.py on {torch.cuda.get_device_name(0)}: 12 layers, V = {V}, block 1024, prompt {args.prompt}, temperature 0.8; step time from calls "
        f"of {BASE} and {BASE + args.steps} tokens; device-event time, one warm-up, median of {args.reps} [min .. max]")
    say(f"parent library: {'given' if parent else 'not given (the off line is the same launches)'}")
    say(f"one walk of a row: {V} floats = {V * 4 / 1e3:.0f} KB from L2 at 64 B/clk, 2.4 GHz = {walk_us:.2f} us for the row's one workgroup")
    say()
    rng = np.random.default_rng(11)
    for B in (1, 16, 64):
        prompts = torch.from_numpy(rng.integers(0, V, size=(B, args.prompt)).astype(np.int32)).to(DEV)
        lens = [args.prompt] * B
        d_u = torch.from_numpy(seeded_uniforms(5, B, BASE + args.steps)).to(DEV)
        out = (torch.empty((B, BASE + args.steps), dtype=torch.int32, device=DEV), torch.empty(B, dtype=torch.int32, device=DEV),
               torch.empty(B, dtype=torch.int32, device=DEV))

        def step_us(g, top_k, top_p):
            def run():
                if g is new:
                    _cabi.check(new.lib.at_gpt_set_truncation(new.h, top_p, 0.0), "at_gpt_set_truncation")
                a = once(lambda: g.generate(prompts, lens, BASE, d_u, top_k, out))
                b = once(lambda: g.generate(prompts, lens, BASE + args.steps, d_u, top_k, out))
                if g is new:
                    _cabi.check(new.lib.at_gpt_set_truncation(new.h, 1.0, 0.0), "at_gpt_set_truncation")
                return (b - a) / args.steps * 1e3
            return run

        configs = {}
        if parent:
            configs["parent"] = step_us(parent, 100, 1.0)
        configs["off"] = step_us(new, 100, 1.0)
        configs["top_p 0.9"] = step_us(new, 100, 0.9)
        configs["top_p 0.9, k=V"] = step_us(new, V, 0.9)
        if parent:
            configs["parent, k=V"] = step_us(parent, V, 1.0)
        configs["off, k=V"] = step_us(new, V, 1.0)
        got = measure(configs, args.reps)
        say(f"B = {B}: us per generation step")
        ref = statistics.median(got["parent"]) if parent else None
        med = {}
        for name, xs in got.items():
            med[name], text = line(name, xs, "us", ref if name in ("off", "top_p 0.9") else (statistics.median(got["parent, k=V"]) if parent and "k=V" in name else None))
            say(text)
        say(f"  added by top_p 0.9 at top_k 100: {med['top_p 0.9'] - med['off']:+.2f} us per step (one more walk: {walk_us:.2f} us); "
            f"at top_k = V: {med['top_p 0.9, k=V'] - med['off, k=V']:+.2f} us per step (four more walks: {4 * walk_us:.2f} us)")
        # the sampler alone
        z = torch.from_numpy((rng.standard_normal((B, V)) * 4.0).astype(np.float32)).to(DEV)
        u1 = d_u[:, 0].contiguous()
        tok = torch.empty(B, dtype=torch.int32, device=DEV)
        stream = _cabi.current_stream_handle(DEV)

        def op_us(lib, top_k, top_p):
            def call():
                for _ in range(20):
                    if top_p is None:
                        rc = lib.at_op_topk_sample(z.data_ptr(), B, V, 0.8, top_k, u1.data_ptr(), None, tok.data_ptr(), stream)
                    else:
                        rc = lib.at_op_nucleus_sample(z.data_ptr(), B, V, 0.8, top_k, top_p, 0.0, u1.data_ptr(), None, tok.data_ptr(), None, None, stream)
                    assert rc == 0
            return lambda: once(call) / 20 * 1e3

        ops = {}
        if parent:
            ops["parent"] = op_us(parent.lib, 100, None)
        ops["off"] = op_us(new.lib, 100, None)
        ops["top_p 0.9"] = op_us(new.lib, 100, 0.9)
        ops["top_p 0.9, k=V"] = op_us(new.lib, V, 0.9)
        ops["off, k=V"] = op_us(new.lib, V, None)
        got = measure(ops, args.reps)
        say(f"B = {B}: us per sampler launch alone (20 back-to-back launches per timing)")
        ref = statistics.median(got["parent"]) if parent else None
        for name, xs in got.items():
            say(line(name, xs, "us", ref if name == "off" else None)[1])
        say()
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "nucleus.txt"), "w") as f:
        f.write("\n".join(LINES) + "\n")
    print(f"wrote {out_dir}/nucleus.txt")


if __name__ == "__main__":
    main()
