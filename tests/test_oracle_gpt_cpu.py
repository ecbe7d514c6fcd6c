"""CPU: the GPT twin (tests/gpt_ref.py), which every GPU test of the semantic-to-acoustic decoder leans on, against vectors recorded from the reference's
own ``gpt2_model.py`` and ``decoder.py`` (tests/golden/gpt_a.npz, made by tests/golden/make_golden.py gpt): the forward, the sampling rule step by step
against the reference's ``generate`` loop, ties at the top-k threshold, the stop token, the prompt layout and the deserialisation. Then the proof that
the GPU bar has power at the long-context inputs the GPU file uses: deliberately wrong twins move the compared logits by many times the bar."""
import os

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.configs import Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import coarse_codes, prepare_source, seeded_uniforms

from tests import gpt_edge_cases as EC
from tests import gpt_ref as R
from tests.parity import FLOAT_TOL

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gpt_a.npz"))
FAMILIES = ["uniform", "peaky"]


@pytest.fixture(scope="module")
def small_models():
    return {f: W.synth_gpt_weights(n_layer=int(GOLD["n_layer"]), vocab=int(GOLD["vocab"]), block=int(GOLD["block"]), seed=int(GOLD["weight_seed"]), family=f)
            for f in FAMILIES}


@pytest.mark.parametrize("family", FAMILIES)
def test_twin_forward_against_the_reference(small_models, family):
    """The reference's fp32 last-position logits of one id sequence cut at T = 1, 64, 65, 257, 513, 1024: causal, so one forward of the 1024 gives them all."""
    ids = np.random.default_rng(int(GOLD["ids_seed"])).integers(0, int(GOLD["vocab"]), size=1024)
    lengths = GOLD["lengths"].tolist()
    assert lengths == [1, 64, 65, 257, 513, 1024]
    got = R.forward(small_models[family], ids, torch.float64, positions=[T - 1 for T in lengths]).numpy()
    diff = np.abs(got - GOLD[f"logits_{family}"].astype(np.float64)).max(axis=1)
    print(f"{family}: twin float64 against the reference's fp32 logits: {diff.max():.2e} (largest |logit| {np.abs(got).max():.1f})")
    assert diff.max() < 1e-4, dict(zip(lengths, diff.tolist()))


@pytest.mark.parametrize("run", ["free", "stop", "tie"])
@pytest.mark.parametrize("family", FAMILIES)
def test_sampling_rule_against_the_reference_generate(small_models, family, run):
    """Teacher-forced on the sequence the reference's generate loop returned (its temperature, top-k masking, ties, softmax and stop handling; the draw
    alone is this project's): the twin's rule on the twin's float32 logits gives the same token at every step, and at the first 4 steps the same kept
    set and the same probabilities. The fixture's draws lie at least 1e-3 from every CDF boundary."""
    w = small_models[family]
    if run == "tie":   # the fixture's tie: one wte row overwritten with another, so the two ids share a logit
        src, dst = GOLD[f"tie_{family}"].tolist()
        w = dict(w)
        w["transformer.wte.weight"] = w["transformer.wte.weight"].copy()
        w["transformer.wte.weight"][dst] = w["transformer.wte.weight"][src]
    P, steps, temperature, top_k = int(GOLD["prompt_len"]), int(GOLD["steps"]), float(GOLD["temperature"]), int(GOLD["top_k"])
    seq, stop, probs = GOLD[f"seq_{family}_{run}"], int(GOLD[f"stop_{family}_{run}"]), GOLD[f"probs_{family}_{run}"]
    u = seeded_uniforms(int(GOLD[f"draw_seed_{family}_{run}"]), 1, steps)[0]
    assert float(GOLD["closest_boundary"]) >= 1e-3
    n = len(seq) - P
    want = seq[P:].tolist()
    if run == "stop":
        free = GOLD[f"seq_{family}_free"]
        assert stop == int(free[P + 7]) and n < steps
        assert want == free[P:].tolist()[:free[P:].tolist().index(stop)], "the sequence ends before the first stop token, which is not emitted"
        want = want + [stop]       # the step that drew it
    else:
        assert n == steps
    logits = R.forward(w, seq, torch.float32, positions=list(range(P - 1, P - 1 + len(want)))).numpy()
    assert logits.shape[0] == len(want)
    for s, tok in enumerate(want):
        assert R.sample(logits[s], temperature, top_k, u[s])[0] == tok, (s, tok)
        if s < probs.shape[0]:
            kept, weights = R.kept_weights(logits[s], temperature, top_k)
            assert np.array_equal(kept, np.nonzero(probs[s])[0]), f"step {s}: the kept set differs from the reference's"
            assert np.abs(weights - probs[s][kept]).max() <= 1e-6
    if run == "tie":
        kept, _ = R.kept_weights(logits[0], temperature, top_k)
        assert kept.size == top_k + 1 and {src, dst} <= set(kept.tolist()), "both ids of a tie at the threshold stay"


def test_helpers_against_the_reference():
    """decoder.py's _prepare_source (the reference appends the INFER token afterwards, in forward), _extract_new_tokens and _deserialize_acoustic_tokens."""
    cfg = Wav2VecBertDecoderConfig()
    for name in ("2d", "long"):
        p = prepare_source(GOLD[f"src_{name}"], cfg)
        assert p[-1] == cfg.INFER_TOKEN and np.array_equal(p[:-1], GOLD[f"prepared_{name}"][0])
    assert GOLD["prepared_long"].shape == (1, cfg.max_source_tokens)
    for name in ("stop", "free"):
        y = GOLD[f"y_{name}"].tolist()
        new = y[y.index(cfg.INFER_TOKEN) + 1:]            # what generate returns after the prompt; a stop token ends it and is not part of it
        if cfg.STOP_TOKEN in new:
            new = new[:new.index(cfg.STOP_TOKEN)]
        assert new == GOLD[f"new_{name}"].tolist()
        assert np.array_equal(coarse_codes(np.array(new) - cfg.ACOUSTIC_OFFSET).numpy(), GOLD[f"codes_{name}"])
    assert cfg.STOP_TOKEN in GOLD["y_stop"] and cfg.STOP_TOKEN not in GOLD["y_free"]


def test_fallback_never_returns_a_zero_weight_id():
    """A top_k past the finite ids makes the threshold -inf and keeps every id; at u = 1 no running sum exceeds u S (weights that are powers of two: every
    sum is exact), and the fallback is the highest kept id that is not -inf."""
    ninf = -np.inf
    tok, _, kept = R.sample(np.array([0.0, 1.0, ninf], dtype=np.float32), 1.0, 100, 1.0)
    assert (tok, kept) == (1, 3)
    z = np.full(65, ninf, dtype=np.float32)
    z[[3, 40]] = [0.0, np.log(2.0)]
    assert R.sample(z, 1.0, 65, 1.0)[0] == 40 and R.sample(z, 1.0, 2, 1.0)[0] == 40
    assert R.sample(np.zeros(4, dtype=np.float32), 1.0, 4, 1.0, allow=(0, 2, 0, 0))[0] == 1
    assert R.sample(np.zeros(4, dtype=np.float32), 1.0, 4, 1.0)[0] == 3, "finite ids: the highest kept id, as before"


# ---- the GPU bar has power at the long-context inputs ---------------------------------------------------------------------------------------------
def _mutant(kind, *args):
    """A deliberately wrong twin: (a replacement for gpt_ref.causal_attention or None, a map over the weights or None)."""
    right = R.causal_attention
    if kind == "mask":
        qi, kj = args

        def attention(q, k, v):     # that query does not see that key
            out = right(q, k, v).clone()
            s = (q[:, qi:qi + 1] @ k[:, :qi + 1].transpose(-1, -2)) * 0.125
            s[..., kj] = float("-inf")
            out[:, qi:qi + 1] = torch.softmax(s, dim=-1) @ v[:, :qi + 1]
            return out
        return attention, None
    if kind == "kv":
        j, = args

        def attention(q, k, v):     # that token's K and V were never written
            k, v = k.clone(), v.clone()
            k[:, j] = 0
            v[:, j] = 0
            return right(q, k, v)
        return attention, None
    p, = args

    def weights(w):                 # every position from p on takes the next one's embedding
        w = dict(w)
        wpe = w["transformer.wpe.weight"]
        w["transformer.wpe.weight"] = np.concatenate([wpe[:p], wpe[p + 1:], wpe[-1:]])
        return w
    return None, weights


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", list(EC.LONG_CASES))
def test_gpu_bar_has_power_at_the_long_context_inputs(small_models, monkeypatch, case, family):
    """At the ids and positions the GPU long-context tests compare, each wrong twin moves the logits by at least 5 FLOAT_TOL: a kernel with that error
    cannot pass them."""
    seq, positions = EC.long_sequence(case)
    w = small_models[family]
    base = R.forward(w, seq, torch.float64, positions=positions)
    for mutant in EC.LONG_CASES[case]["mutants"]:
        attention, weights = _mutant(*mutant)
        with monkeypatch.context() as m:
            if attention:
                m.setattr(R, "causal_attention", attention)
            shift = float((R.forward(weights(w) if weights else w, seq, torch.float64, positions=positions) - base).abs().max())
        print(f"{case} {family} {mutant}: shifts the compared logits by {shift:.2e}")
        assert shift >= 5 * FLOAT_TOL, (case, family, mutant, shift)
