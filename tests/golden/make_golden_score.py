"""Generate tests/golden/gpt_score_a.npz (run in the BUILD container only: needs read access to /root/reference).

    python tests/golden/make_golden_score.py

The reference's GPT (gpt2_model.py: get_model(n_layer=2, vocab_size=2048, block_size=1024), bias-free) loaded with the synthetic weights of both families,
run through the half of its ``forward`` that generation never takes: ``forward(idx, targets)``, logits at every position and
``F.cross_entropy(..., ignore_index=-1)``. A sequence of L ids (L = 2, 65, 257, 1024, cuts of one seeded id sequence) gives ``idx = ids[:L - 1]`` and
``targets = ids[1:]``, with the targets before ``score_from - 1`` set to -1, so that ``ignore_index`` is exercised. Recorded per family and length, results
only: the reference's ``loss``; at every position that is not ignored, the ``log_softmax`` of its logits gathered at the target, the count of logits above
the target's, and the count of other ids whose logit lies within 2 FLOAT_TOL of the target's (where a second implementation's rank may differ)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

from audiotoken_amd import weights as W  # noqa: E402
from make_golden import GPT_IDS_SEED, GPT_V, _gpt_model  # noqa: E402
from tests.parity import FLOAT_TOL  # noqa: E402

LENGTHS = (2, 65, 257, 1024)
SCORE_FROM = (1, 22, 129, 1000)   # the first scored position of each length: nothing ignored, a third, a half, all but the last 24


def make_score():
    from _ref_gpt_loader import load_reference_gpt
    G = load_reference_gpt()["gpt2_model"]
    seq = np.random.default_rng(GPT_IDS_SEED).integers(0, GPT_V, size=1024)
    out = dict(ids_seed=GPT_IDS_SEED, lengths=np.array(LENGTHS), score_from=np.array(SCORE_FROM), weight_seed=0, n_layer=2, vocab=GPT_V, block=1024)
    for family in ("uniform", "peaky"):
        model = _gpt_model(G, W.synth_gpt_weights(n_layer=2, vocab=GPT_V, block=1024, seed=0, family=family))
        for L, first in zip(LENGTHS, SCORE_FROM):
            ids = torch.from_numpy(seq[:L].astype(np.int64))
            targets = ids[1:].clone()
            targets[:first - 1] = -1
            with torch.no_grad():
                logits, loss = model(ids[None, :L - 1], targets[None])
            z = logits[0, first - 1:]                                   # the positions that are not ignored
            t = ids[first:]
            zt = z.gather(1, t[:, None])
            out[f"loss_{family}_{L}"] = np.float32(loss.item())
            out[f"logprob_{family}_{L}"] = torch.log_softmax(z, dim=-1).gather(1, t[:, None])[:, 0].numpy().copy()
            out[f"rank_{family}_{L}"] = (z > zt).sum(dim=1).numpy().astype(np.int32)
            out[f"near_{family}_{L}"] = ((z - zt).abs() <= 2 * FLOAT_TOL).sum(dim=1).numpy().astype(np.int32) - 1   # the target itself is not counted
    np.savez_compressed(os.path.join(HERE, "gpt_score_a.npz"), **out)
    print("gpt_score", {k: np.asarray(v).shape for k, v in out.items()})


if __name__ == "__main__":
    torch.manual_seed(0)
    make_score()
