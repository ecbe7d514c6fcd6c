"""CPU: the scoring twin (tests/gpt_score_ref.py), which every GPU test of teacher-forced scoring leans on, against vectors recorded from the half of the
reference's ``GPT.forward`` that generation never takes: ``forward(idx, targets)`` with ``F.cross_entropy(..., ignore_index=-1)``
(tests/golden/gpt_score_a.npz, made by tests/golden/make_golden_score.py). Then the proof that the bar has power: a twin with its targets shifted by one,
and one that scores position p on the logits of position p, miss the golden by many times the bar."""
import os

import numpy as np
import pytest

from audiotoken_amd import weights as W

from tests import gpt_score_ref as SR
from tests.parity import FLOAT_TOL

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt_score_a.npz"))
FAMILIES = ["uniform", "peaky"]
CASES = list(zip(GOLD["lengths"].tolist(), GOLD["score_from"].tolist()))


@pytest.fixture(scope="module")
def small_models():
    return {f: W.synth_gpt_weights(n_layer=int(GOLD["n_layer"]), vocab=int(GOLD["vocab"]), block=int(GOLD["block"]), seed=int(GOLD["weight_seed"]), family=f)
            for f in FAMILIES}


def sequence(L):
    return np.random.default_rng(int(GOLD["ids_seed"])).integers(0, int(GOLD["vocab"]), size=1024)[:L]


@pytest.fixture(scope="module")
def twin_scores(small_models):
    """The twin's scores of every case, computed once."""
    return {(f, L): SR.score_sequence(small_models[f], sequence(L), first)[:2] for f in FAMILIES for L, first in CASES}


def test_the_cases_are_the_issue_s():
    assert [L for L, _ in CASES] == [2, 65, 257, 1024]
    assert CASES[0][1] == 1 and all(first > 1 for _, first in CASES[1:]), "a prefix of the targets is ignored wherever the sequence has one"


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L,first", CASES)
def test_twin_scores_against_the_reference(twin_scores, family, L, first):
    lp, rank = twin_scores[(family, L)]
    want = GOLD[f"logprob_{family}_{L}"].astype(np.float64)
    assert lp.shape == want.shape == (L - first,)
    diff = np.abs(lp - want).max()
    loss = abs(-lp.mean() - float(GOLD[f"loss_{family}_{L}"]))
    print(f"{family} L={L}: log-probs differ from the reference's by {diff:.2e}, the mean from its loss by {loss:.2e}")
    assert diff <= FLOAT_TOL
    assert loss <= FLOAT_TOL, "-mean over the positions that are not ignored is the reference's cross-entropy"
    # equal, or the recorded logits put that many ids within 2 FLOAT_TOL of the target's
    off = np.abs(rank - GOLD[f"rank_{family}_{L}"])
    assert bool((off <= GOLD[f"near_{family}_{L}"]).all()), (off, GOLD[f"near_{family}_{L}"])
    print(f"{family} L={L}: {int((off > 0).sum())} of {off.size} ranks differ, all at recorded near-ties")


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("L,first", CASES[1:])
def test_the_bar_has_power_against_shifted_targets_and_positions(small_models, family, L, first):
    """Two wrong twins: the targets taken one position late (ids[p + 1] scored where ids[p] belongs), and position p scored on the logits of position p
    instead of p - 1. Each must miss the golden's per-position log-probs, which is what the bar is applied to, by more than 8 times the bar. The mean is
    printed and not asserted: on random targets a model close to uniform gives every id about -ln V, so a mean over other positions' values hardly moves."""
    w, ids = small_models[family], sequence(L)
    want = GOLD[f"logprob_{family}_{L}"].astype(np.float64)
    # (the shifted targets are also the model's later inputs; the first scored position sees only true inputs, and it is asserted on its own below)
    late = SR.score_sequence(w, np.concatenate([ids[:first], ids[first + 1:], ids[first:first + 1]]), first)[0]
    same_pos = SR.score_sequence(w, ids, first, at=lambda p: p)[0]
    for name, got in (("targets shifted by one", late), ("position p instead of p - 1", same_pos)):
        miss, loss = np.abs(got - want).max(), abs(-got.mean() - float(GOLD[f"loss_{family}_{L}"]))
        print(f"{family} L={L} {name}: misses the log-probs by {miss:.2e}, the loss by {loss:.2e}")
        assert miss > 8 * FLOAT_TOL, (name, miss)
    assert abs(late[0] - want[0]) > 8 * FLOAT_TOL, "the first scored position sees true inputs and a wrong target"
