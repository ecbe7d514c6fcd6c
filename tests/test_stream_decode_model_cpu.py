"""CPU: the streaming decode algorithm (tests/stream_decode_ref.py), pushed by several schedules, against the oracle's one-shot decode.
The bar is tests/parity.py FLOAT_TOL on the max-abs difference. A control with ONE context frame must miss the bar: an output sample reaches
back to row floor(n / 320) - 2 of the upsampling stack's input (final conv 6 samples; per stage the block's k3 conv 2 rows and the
transposed conv 1 input row)."""
import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from oracle import encodec_ref as R
from tests import parity as P
from tests.stream_decode_ref import stream_decode

B, K, T = 2, 8, 40


@pytest.fixture(scope="module")
def weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True)


@pytest.fixture(scope="module")
def tokens():
    return torch.randint(0, 1024, (B, K, T), dtype=torch.long, generator=torch.Generator().manual_seed(4))


@pytest.fixture(scope="module")
def one_shot(weights, tokens):
    return R.acoustic_decode(weights, tokens).reshape(B, 320 * T)


def _random_schedule(seed):
    rng = np.random.default_rng(seed)
    out = [int(rng.integers(7, 12))]
    while sum(out) < T:
        out.append(int(rng.integers(1, 9)))
    return out


SCHEDULES = {
    "seven_then_single": [7] + [1] * (T - 7),
    "ragged": [7, 3, 10, 1, 19],
    "one_push": [T],
    "halves": [20, 20],
    "random": _random_schedule(5),
}


@pytest.mark.parametrize("name", sorted(SCHEDULES))
def test_context_two_reproduces_one_shot(weights, tokens, one_shot, name):
    got = stream_decode(weights, tokens, SCHEDULES[name], context_frames=2)
    assert got.shape == one_shot.shape
    err = (got - one_shot).abs().max().item()
    print(f"{name}: max |stream - one-shot| = {err:.3e} at waveform scale {one_shot.abs().max().item():.2f}")
    assert err < P.FLOAT_TOL, f"{name}: waveform difference {err}"


@pytest.mark.parametrize("name", ("seven_then_single", "ragged", "halves"))
def test_context_one_is_too_short(weights, tokens, one_shot, name):
    got = stream_decode(weights, tokens, SCHEDULES[name], context_frames=1)
    err = (got - one_shot).abs().max().item()
    print(f"{name}, ONE context frame: max |stream - one-shot| = {err:.3e}")
    assert err > P.FLOAT_TOL
