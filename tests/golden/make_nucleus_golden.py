"""Maker of tests/golden/nucleus_a.npz: the kept masks of Hugging Face's logits warpers on small random rows, for tests/test_nucleus_cpu.py to hold the
twin (tests/nucleus_ref.py) against. Needs ``transformers``; stores inputs and results only.

    python tests/golden/make_nucleus_golden.py

Per case: fp32 logits ``[6, 512]``, then ``TemperatureLogitsWarper``, ``TopKLogitsWarper``, ``TopPLogitsWarper`` and ``MinPLogitsWarper`` in the order
``generate`` chains them (a warper whose value is off is left out); the mask is where the result is finite."""
import os

import numpy as np
import torch
from transformers.generation.logits_process import MinPLogitsWarper, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = [  # temperature, top_k, top_p (1: off), min_p (0: off)
    (1.0, 512, 0.9, 0.0), (0.8, 512, 0.3, 0.0), (0.8, 100, 0.9, 0.0), (1.0, 100, 0.5, 0.05), (0.8, 20, 0.95, 0.0), (1.0, 512, 1.0, 0.05),
    (0.8, 100, 1.0, 0.2), (0.8, 100, 0.99, 0.01), (2.0, 50, 0.7, 0.1),
]


def main():
    out = {"cases": np.asarray(CASES, dtype=np.float64)}
    for i, (T, k, p, q) in enumerate(CASES):
        z = (np.random.default_rng(500 + i).standard_normal((6, 512)) * 3.0).astype(np.float32)
        s = torch.from_numpy(z.copy())
        ids = torch.zeros((6, 1), dtype=torch.long)
        if T != 1.0:
            s = TemperatureLogitsWarper(float(T))(ids, s)
        s = TopKLogitsWarper(int(k))(ids, s)
        if p < 1.0:
            s = TopPLogitsWarper(float(p))(ids, s)
        if q > 0.0:
            s = MinPLogitsWarper(float(q))(ids, s)
        out[f"logits_{i}"] = z
        out[f"mask_{i}"] = torch.isfinite(s).numpy()
    np.savez_compressed(os.path.join(HERE, "nucleus_a.npz"), **out)
    print("wrote nucleus_a.npz:", {k: v.shape for k, v in out.items() if k.startswith("mask")})


if __name__ == "__main__":
    main()
