"""What tests/test_fine_decoder_gpu.py runs and tests/test_fine_decoder_cpu.py qualifies without a device, in one place so that both use the very same
models, rows and draws."""
import numpy as np

from audiotoken_amd import weights as W
from audiotoken_amd.fine_decoder import seeded_uniforms

# the two small models of tests/golden/make_golden_fine.py
MODELS = {"a": dict(block=128, n_layer=2, hidden=768, bias=False), "b": dict(block=256, n_layer=1, hidden=1024, bias=True)}
FAMILIES = ("uniform", "peaky")
SEED = 2024           # the draws of every GPU test; the CPU file shows that the twin's own generation leaves them off the CDF boundaries
TEMPERATURE = 0.5     # bark's default
WAIVER_CAP = 0.02     # of a test's draws

_weights = {}


def weights(m, family):
    if (m, family) not in _weights:
        k = MODELS[m]
        _weights[(m, family)] = W.synth_fine_weights(k["n_layer"], k["hidden"], k["block"], seed=0, family=family, bias=k["bias"])
    return _weights[(m, family)]


def lengths(block):
    """The golden list: every T at which the schedule changes."""
    H = block // 2
    return [1, H, block - 1, block, block + 1, block + H, block + H + 1, 2 * block + 3]


def coarse_row(T, seed=0):
    return np.random.default_rng(7919 * seed + T).integers(0, 1024, size=(2, T))


def draws(rows, block, seed=SEED):
    """float32 [B, n_max, 6, W] for rows of the given lengths."""
    H = block // 2
    n_max = max(max(0, -(-(T - block) // H)) + 1 for T in rows)
    return seeded_uniforms(seed, len(rows), n_max, block)


# The lost-key case: model a, peaky, one full window (T = W, so that every key is a real frame) and the first pass (code book 2), whose buffer is the
# coarse input alone and therefore known without a device. The CPU file shows that the twin without its last 64 keys (the attention kernel's key tile)
# moves these logits by more than 8 times the float bar; the GPU file compares exactly these logits against the bar.
LOST_KEY = dict(model="a", family="peaky", T=128, keys=64, seed=5)
