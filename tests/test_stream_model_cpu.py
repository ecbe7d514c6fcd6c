"""CPU: the streaming-encode algorithm (tests/stream_ref.py: carried context samples, LSTM state and final-conv history) against the
oracle's one-shot encode. The bar is the project's standing one: embeddings within FLOAT_TOL, ids equal or explained by an oracle
near-tie. A control with ONE context frame must miss the bar — the receptive field of a frame reaches 478 samples back."""
import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from oracle import encodec_ref as R
from tests import parity as P
from tests import stream_ref as S

N_Q = 8


@pytest.fixture(scope="module")
def weights():
    return W.synth_encodec_weights(seed=0, with_decoder=False)


def _wav(B, N, seed=7):
    return torch.from_numpy(W.synth_waveform(B, N, 24000, seed=seed))


def _random_schedule(total, seed):
    rng = np.random.default_rng(seed)
    out, pos = [], 0
    while pos < total:
        n = int(rng.integers(1, 4000))
        out.append(n)
        pos += n
    return out


def _check(w, wav, schedule, what, context_frames=2):
    emb = S.stream_encode(w, wav, schedule, context_frames)
    ref = R.seanet_encode(w, wav)
    assert emb.shape == ref.shape, (emb.shape, ref.shape)
    err = (emb - ref).abs().max().item()
    print(f"{what}: max |stream - one-shot| embedding difference {err:.3e}")
    assert err < P.FLOAT_TOL, f"{what}: embedding difference {err}"
    ref_codes, margins = R.acoustic_encode(w, wav, N_Q, return_margins=True)
    codes = R.rvq_encode(w, emb, N_Q).transpose(0, 1).to(torch.int16)
    P.assert_rvq_equal_or_explained(codes, ref_codes, margins, P.RVQ_TIE, what)
    return err


SCHEDULES = {
    "one_push": lambda total: [total],
    "hop_320": lambda total: [320] * (total // 320 + 1),
    "hop_6400": lambda total: [6400] * (total // 6400 + 1),
    "random": lambda total: _random_schedule(total, 11),
}


@pytest.mark.parametrize("tail", [0, 1, 9, 319])
@pytest.mark.parametrize("schedule", sorted(SCHEDULES))
def test_stream_model_equals_one_shot(weights, schedule, tail):
    total = 40 * 320 + tail
    _check(weights, _wav(1, total), SCHEDULES[schedule](total), f"{schedule}, tail {tail}")


def test_stream_model_batch_of_three(weights):
    total = 30 * 320 + 9
    _check(weights, _wav(3, total, seed=3), _random_schedule(total, 5), "B = 3, random schedule")


def test_stream_shorter_than_first_push_minimum_is_one_shot(weights):
    total = 3 * 320 + 9   # below the first push's minimum: everything is held and flush() encodes it one-shot
    wav = _wav(1, total)
    emb = S.stream_encode(weights, wav, [320] * 4)
    assert torch.equal(emb, R.seanet_encode(weights, wav))


def test_one_context_frame_misses_the_bar(weights):
    """The control: with 320 samples of context the first kept frame of a push has seen reflected samples instead of its history."""
    total = 40 * 320
    wav = _wav(1, total)
    emb = S.stream_encode(weights, wav, [6400] * 7, context_frames=1)
    err = (emb - R.seanet_encode(weights, wav)).abs().max().item()
    print(f"one context frame: max embedding difference {err:.3e}")
    assert err > P.FLOAT_TOL
