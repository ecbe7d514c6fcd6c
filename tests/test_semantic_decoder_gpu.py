"""GPU: the KV-cached GPT decoder (csrc/gpt.hip, audiotoken_amd/semantic_decoder.py) against the CPU twin in tests/gpt_ref.py.

The protocol (``verify_generation``): the twin runs ONCE per row, teacher-forced on the device's own sequence. (a) every device logit vector is within
``parity.FLOAT_TOL`` of the twin's float64 logits at that position; (b) the device's token equals ``gpt_ref.sample`` applied to the DEVICE's logits with
the same draw, waived only where the draw lies within 2 (kept 2^-24 + 2^-22) of a CDF boundary (the worst case of ``kept`` sequential fp32 additions
plus a 2-ulp expf, on both sides), for at most 2 % of a test's steps; (c) the rows end as the finish rules say and nothing is written past a row's
length. Both (a) and (b) are anchored on the device's sequence, so a near-tie cannot cascade and a wrong token cannot hide."""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import weights as W
from audiotoken_amd.configs import Tokenizers, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, seeded_uniforms, topk_sample

from tests import gpt_ref as R
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V_SMALL = 2048
SEED = 2024          # tests/test_semantic_decoder_cpu.py checks that this seed keeps the twin's own generation away from the CDF boundaries
CFG = Wav2VecBertDecoderConfig()
RECORD = {"max_logit_diff": 0.0, "waived": 0, "steps": 0}


def window(kept):
    return 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)


_models = {}


def model(family="uniform", block=1024):
    """(weights, decoder) of the 2-layer model with a 2048-id vocabulary."""
    key = (family, block)
    if key not in _models:
        w = W.synth_gpt_weights(n_layer=2, vocab=V_SMALL, block=block, seed=0, family=family)
        _models[key] = (w, SemanticToAcoustic(device=DEV, weights=w))
    return _models[key]


def big_weights():
    """The full-size model's weights (12 layers, 53376 ids), made once; ``big2`` is its first two layers."""
    if "big" not in _models:
        _models["big"] = W.synth_gpt_weights(n_layer=12, vocab=CFG.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    return _models["big"]


def big2():
    if "big2" not in _models:
        w = {k: v for k, v in big_weights().items() if not k.startswith("transformer.h.") or int(k.split(".")[2]) < 2}
        _models["big2"] = (w, SemanticToAcoustic(CFG, device=DEV, weights=w))
    return _models["big2"]


def prompts_of(lengths, vocab, seed=7):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, vocab, size=n).astype(np.int32) for n in lengths]


def verify_generation(w, dec, prompts, ids, finish, logits, uniforms, temperature, top_k, stop_token, max_new, allow=None):
    block = dec.block_size
    raw = dec.last_raw_ids
    waived = steps = 0
    worst = 0.0
    for b, prompt in enumerate(prompts):
        P, n = len(prompt), len(ids[b])
        L = logits[b].numpy()
        stopped = finish[b] == "stop"
        # (c) structure
        assert L.shape[0] == n + (1 if stopped else 0)
        assert stop_token not in ids[b].tolist(), "the stop token is not emitted"
        if stopped:
            assert n < max_new and P + n < block
        elif finish[b] == "max_new_tokens":
            assert n == max_new and (P + n <= block)
        else:
            assert finish[b] == "block_size" and P + n == block and n < max_new
        assert np.array_equal(raw[b, :n].numpy(), ids[b].numpy()) and bool((raw[b, n:] == -1).all()), "nothing is written past a row's length"
        # (a) the float bar, teacher-forced on the device's sequence
        seq = np.concatenate([prompt, ids[b].numpy()])
        ref = R.forward(w, seq, torch.float64, positions=list(range(P - 1, P - 1 + L.shape[0]))).numpy()
        diff = float(np.abs(L.astype(np.float64) - ref).max())
        worst = max(worst, diff)
        assert diff <= FLOAT_TOL, f"row {b}: logits differ from the float64 twin by {diff:.3e}"
        # (b) the sampler, exactly, on the device's logits
        for s in range(L.shape[0]):
            want = int(ids[b][s]) if s < n else stop_token
            tok, dist, kept = R.sample(L[s], temperature, top_k, uniforms[b, s], None if allow is None else allow[s % 2])
            steps += 1
            if tok != want:
                assert dist < window(kept), f"row {b} step {s}: device token {want}, rule gives {tok}, {dist:.3e} from a boundary (window {window(kept):.3e})"
                waived += 1
    print(f"largest logit difference {worst:.3e}; waived {waived} of {steps} steps")
    RECORD["max_logit_diff"] = max(RECORD["max_logit_diff"], worst)
    RECORD["waived"] += waived
    RECORD["steps"] += steps
    assert waived <= 0.02 * steps
    return worst, waived


def run(w, dec, prompts, max_new, stop_token=-1, temperature=0.8, top_k=100, allow=None, seed=SEED):
    u = seeded_uniforms(seed, len(prompts), max_new)
    ids, finish, logits = dec.generate(prompts, max_new, temperature, top_k, stop_token, uniforms=u, allow=allow, return_logits=True)
    verify_generation(w, dec, prompts, ids, finish, logits, u, temperature, top_k, stop_token, max_new, allow)
    return ids, finish


@pytest.mark.parametrize("family", ["uniform", "peaky"])
@pytest.mark.parametrize("plen", [1, 63, 64, 65, 251])
def test_single_row_across_cache_boundaries(family, plen):
    w, dec = model(family)
    ids, finish = run(w, dec, prompts_of([plen], V_SMALL, seed=plen), 80)
    assert finish == ["max_new_tokens"] and len(ids[0]) == 80


@pytest.fixture(scope="module")
def three_rows():
    w, dec = model("peaky")
    prompts = prompts_of([1, 64, 251], V_SMALL)
    ids, finish = run(w, dec, prompts, 80)
    return prompts, ids, finish


def test_three_rows_of_different_lengths(three_rows):
    _, ids, finish = three_rows
    assert finish == ["max_new_tokens"] * 3 and [len(i) for i in ids] == [80] * 3


def test_a_row_stops_and_the_others_go_on(three_rows):
    w, dec = model("peaky")
    prompts, before, _ = three_rows
    stop = int(before[1][7])
    ids, finish = run(w, dec, prompts, 80, stop_token=stop)
    end = before[1].tolist().index(stop)
    assert finish[1] == "stop" and ids[1].tolist() == before[1].tolist()[:end]
    for b in (0, 2):
        if stop not in before[b].tolist():
            assert finish[b] == "max_new_tokens" and torch.equal(ids[b], before[b]), "a finished row must not disturb the others"


def test_seventeen_rows_more_than_one_pass():
    w, dec = model("uniform")
    ids, finish = run(w, dec, prompts_of([5] * 17, V_SMALL), 8)
    assert finish == ["max_new_tokens"] * 17
    assert len({tuple(i.tolist()) for i in ids}) > 1, "rows with different prompts and draws"


def test_block_size_finish():
    w, dec = model("uniform", block=128)
    ids, finish = run(w, dec, prompts_of([100], V_SMALL), 64)
    assert finish == ["block_size"] and len(ids[0]) == 28


def test_constrained_steps_stay_in_their_code_book():
    w, dec = big2()
    a, n, stop = CFG.ACOUSTIC_OFFSET, 1024, CFG.STOP_TOKEN
    allow = [[a, a + n, stop, stop + 1], [a + n, a + 2 * n, 0, 0]]
    prompts = prompts_of([30, 9], CFG.VOCAB_SIZE)
    ids, finish = run(w, dec, prompts, 24, stop_token=stop, allow=allow)
    for b in range(2):
        for s, t in enumerate(ids[b].tolist()):
            assert a + n * (s % 2) <= t < a + n * (s % 2 + 1), (b, s, t)
        if finish[b] == "stop":
            assert len(ids[b]) % 2 == 0, "STOP only at even steps"


def test_full_size_shape():
    w = big_weights()
    dec = SemanticToAcoustic(CFG, device=DEV, weights=w)
    assert (dec.n_layers, dec.vocab, dec.block_size) == (12, 53376, 1024)
    run(w, dec, prompts_of([251, 251], CFG.VOCAB_SIZE), 32)


# ---- the sampler alone ------------------------------------------------------------------------------------------------------------------------
def sampler_case(z, temperature, top_k, u, allow=None):
    """Exact equality with the rule on logits whose draws the test first shows to be far from every boundary."""
    z = np.ascontiguousarray(z, dtype=np.float32)
    u = np.asarray(u, dtype=np.float32)
    want = []
    for b in range(z.shape[0]):
        tok, dist, _ = R.sample(z[b], temperature, top_k, u[b], allow)
        assert dist > 1e-4, f"the test's own input: row {b} is {dist:.3e} from a boundary"
        want.append(tok)
    zd, ud = torch.from_numpy(z).to(DEV), torch.from_numpy(u).to(DEV)
    got = topk_sample(zd, temperature, top_k, ud, allow).cpu().tolist()
    again = topk_sample(zd, temperature, top_k, ud, allow).cpu().tolist()
    assert got == want
    assert again == got, "the same call twice gives the same tokens"


def spread_logits(B, V, seed, scale=4.0):
    return (np.random.default_rng(seed).standard_normal((B, V)) * scale).astype(np.float32)


@pytest.mark.parametrize("V", [128, 53376])
@pytest.mark.parametrize("top_k", [1, 100, 1 << 20])
@pytest.mark.parametrize("temperature", [0.8, 1.0])
def test_sampler_against_the_rule(V, top_k, temperature):
    scale = 4.0 if top_k <= 100 or V == 128 else 12.0   # every one of 53376 ids kept: only a peaked row keeps the CDF's large steps apart
    sampler_case(spread_logits(3, V, seed=V + top_k % 97, scale=scale), temperature, top_k, [0.11, 0.52, 0.93])


@pytest.mark.parametrize("V", [128, 53376])
def test_sampler_edges(V):
    z = spread_logits(1, V, seed=3)[0]
    # top_k = 1, the arg-max, whatever the draw; with a tie both ids stay (ties at the threshold are kept) and halve the draw's range: the lowest id below 1/2
    sampler_case(np.stack([z, z]), 1.0, 1, [0.0, 1.0 - 2.0 ** -24])
    t = z.copy(); t[[V // 3, V // 2]] = t.max() + 1.0
    sampler_case(np.stack([t, t, t]), 1.0, 1, [0.0, 0.3, 0.7])
    # five equal values at the threshold of top-3: all kept
    t = z.copy(); t[[5, V // 4, V // 2, V - 9, V - 1]] = t.max() + 0.5; t[7] = t.max() + 1.0; t[V - 2] = t.max() + 0.25
    for u in (0.05, 0.3, 0.45, 0.55, 0.75, 0.9, 0.97):
        sampler_case(t[None], 1.0, 3, [u])
    # rows holding -inf, and a top_k past the finite ids
    t = z.copy(); t[::2] = -np.inf
    sampler_case(np.stack([t, t]), 0.8, 100, [0.2, 0.8])
    t = np.full(V, -np.inf, dtype=np.float32); t[[3, V // 2, V - 1]] = [0.0, 1.0, 0.5]
    sampler_case(t[None], 1.0, 100, [0.5])
    # all-equal logits: the CDF is a ramp of V equal steps; draws at the middle of a step
    t = np.zeros((3, V), dtype=np.float32)
    mids = [(V // 5 + 0.5) / V, (V // 2 + 0.5) / V, (V - 1 + 0.5) / V]
    if V == 128:
        sampler_case(t, 1.0, V, mids)
    # u = 0 and the largest u below 1
    t = z.copy(); t[0] = t[V - 1] = z.max()      # the first and the last kept id carry weight, so that neither draw sits next to a boundary
    sampler_case(np.stack([t, t]), 0.8, 100, [0.0, 1.0 - 2.0 ** -24])
    # an allow range
    sampler_case(np.stack([z, z, z]), 0.8, 100, [0.1, 0.5, 0.9], allow=(V // 4, V // 2, V - 3, V - 2))
    sampler_case(z[None], 1.0, 1, [0.5], allow=(V // 4, V // 2, 0, 0))


# ---- the C ABI's argument checks --------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    w, dec = model("uniform", block=128)
    lib = dec.lib
    B, P, max_new = 2, 8, 4
    prompts = torch.zeros((B, P), dtype=torch.int32, device=DEV)
    u = torch.full((B, max_new), 0.5, device=DEV)
    out = torch.full((B, max_new), -7, dtype=torch.int32, device=DEV)
    n = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    fin = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.at_gpt_state_bytes(dec.handle, B, P + max_new)
    state = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def call(B=B, lens=(P, P), temperature=0.8, top_k=100, state_ptr=state.data_ptr(), stride=P):
        return lib.at_gpt_generate(dec.handle, prompts.data_ptr(), stride, (C.c_int32 * len(lens))(*lens), B, max_new, temperature, top_k, -1, u.data_ptr(),
                                   None, out.data_ptr(), n.data_ptr(), fin.data_ptr(), None, state_ptr, nbytes, P + max_new, _cabi.current_stream_handle(DEV), None)

    for kwargs, text in [(dict(B=0), "B must be"), (dict(B=65), "B must be"), (dict(lens=(P, 129), stride=P), "longer than the model's block"),
                         (dict(top_k=0), "top_k"), (dict(temperature=0.0), "temperature"), (dict(temperature=-1.0), "temperature"),
                         (dict(state_ptr=None), "null state")]:
        assert call(**kwargs) != 0, kwargs
        assert text in _cabi.last_error(), (kwargs, _cabi.last_error())
    assert lib.at_gpt_state_bytes(dec.handle, 0, 16) == 0 and lib.at_gpt_state_bytes(dec.handle, 65, 16) == 0
    torch.cuda.synchronize()
    assert bool((out == -7).all()) and bool((n == -7).all()) and bool((fin == -7).all()) and bool((state == 0).all()), "a refused call writes nothing"
    assert call() == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert n.tolist() == [max_new] * B and fin.tolist() == [2] * B


# ---- the public interface ---------------------------------------------------------------------------------------------------------------------
def test_end_to_end_semantic_ids_to_audio():
    from audiotoken_amd import AudioToken
    w, _ = big2()
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=w)
    tokens = torch.from_numpy(np.random.default_rng(5).integers(0, 1000, size=(1, 60)))
    out = sem.to_acoustic(tokens, constrain=True, max_new_tokens=40, seed=SEED)
    assert out.finish == ["max_new_tokens"] and out.codes[0].shape == (2, 20) and out.codes[0].dtype == torch.int64
    assert int(out.codes[0].min()) >= 0 and int(out.codes[0].max()) < 1024
    audio = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=2).decode(out.codes[0].unsqueeze(0))
    assert audio.shape == (1, 6400) and bool(torch.isfinite(audio).all())


def test_seed_is_reproducible_and_equals_explicit_uniforms():
    from audiotoken_amd import AudioToken
    w, _ = big2()
    sem = AudioToken(Tokenizers.semantic_s, device=DEV, decoder_weights=w)
    tokens = [np.arange(20) % 1000, np.arange(300) % 1000]
    flat = dict(temperature=20.0)   # the peaky family at the default temperature all but decides every step; flattened, the draws matter
    a = sem.to_acoustic(tokens, max_new_tokens=12, seed=3, **flat)
    b = sem.to_acoustic(tokens, max_new_tokens=12, seed=3, **flat)
    c = sem.to_acoustic(tokens, max_new_tokens=12, uniforms=seeded_uniforms(3, 2, 12), **flat)
    d = sem.to_acoustic(tokens, max_new_tokens=12, seed=4, **flat)
    for x in (b, c):
        assert all(torch.equal(p, q) for p, q in zip(a.ids, x.ids)) and a.finish == x.finish
    assert not all(torch.equal(p, q) for p, q in zip(a.ids, d.ids)), "another seed gives other draws"
