"""GPU: the regions of csrc/gpt.hip that tests/test_semantic_decoder_gpu.py leaves unrun, under the same protocol (``verify_generation``: logits within
``parity.FLOAT_TOL`` of the float64 twin, the sampler exact on the device's logits, nothing written past a row's length): a prefill of several rows on the
register-streaming linear path and the switch to the GEMM at 64 / 65 prompt tokens, contexts of more than 512 keys (``gpt_attn_kernel``'s third and
fourth key per thread), more than 17 rows, a row born finished, every row stopping early, an id outside the vocabulary, prompt padding, a reused state
buffer; then the sampler alone at widths that are no multiple of 64, at 1 and 65536, on rows whose top-k threshold the last radix passes decide, and
its fallback. tests/test_oracle_gpt_cpu.py pins the twin to the reference and shows that the long-context inputs used here expose one lost key."""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd.semantic_decoder import seeded_uniforms, topk_sample

from tests import gpt_edge_cases as EC
from tests import gpt_ref as R
from tests.test_semantic_decoder_gpu import DEV, SEED, V_SMALL, model, prompts_of, run, sampler_case, spread_logits, verify_generation

pytestmark = pytest.mark.gpu

FAMILIES = ["uniform", "peaky"]


def checked(w, dec, prompts, max_new, stop_token=-1, temperature=0.8, top_k=100, allow=None, uniforms=None):
    """``run`` of the other file, returning the logits too."""
    u = seeded_uniforms(SEED, len(prompts), max_new) if uniforms is None else uniforms
    ids, finish, logits = dec.generate(prompts, max_new, temperature, top_k, stop_token, uniforms=u, allow=allow, return_logits=True)
    verify_generation(w, dec, prompts, ids, finish, logits, u, temperature, top_k, stop_token, max_new, allow)
    return ids, finish, logits


def same(a, b):
    """Two results of ``checked`` / ``generate``: ids, finish reasons and logits bit for bit."""
    return a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def seeded_lengths(B):
    return np.random.default_rng(B).integers(1, 7, size=B).tolist()


# ---- the prefill's two paths ------------------------------------------------------------------------------------------------------------------
SMALL = [1, 7, 16, 3]


def small_prefill():
    w, dec = model("uniform", block=128)
    return checked(w, dec, prompts_of(SMALL, V_SMALL), 4)


@pytest.fixture(scope="module")
def small_first():
    return small_prefill()


def test_small_prefill_of_several_rows(small_first):
    ids, finish, _ = small_first
    assert finish == ["max_new_tokens"] * 4 and [len(i) for i in ids] == [4] * 4


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("lengths", [[16, 16, 16, 16], [16, 16, 16, 17]], ids=["sum64_linear", "sum65_gemm"])
def test_prefill_path_switch(lengths, family):
    w, dec = model(family, block=128)
    _, finish = run(w, dec, prompts_of(lengths, V_SMALL), 4)
    assert finish == ["max_new_tokens"] * 4


# ---- more than 512 keys -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("case", list(EC.LONG_CASES))
def test_long_context(case, family):
    """The allow ranges force the produced ids (tests/gpt_edge_cases.py), so the inputs are those the CPU file qualified: one lost key moves these logits
    by at least 8 times the bar."""
    c = EC.LONG_CASES[case]
    w, dec = model(family)
    ids, finish = run(w, dec, [EC.long_prompt(c["plen"])], c["max_new"], allow=EC.FORCED_ALLOW)
    seq, _ = EC.long_sequence(case)
    assert ids[0].tolist() == seq[c["plen"]:].tolist()
    assert finish == (["block_size"] if c["plen"] + c["max_new"] > EC.BLOCK else ["max_new_tokens"])
    if case == "longest":
        assert len(ids[0]) == 24, "1000 + 24 ids fill the block; the last step attends 1023 keys"


@pytest.mark.parametrize("family", FAMILIES)
def test_two_long_rows_in_one_call(family):
    w, dec = model(family)
    ids, finish = run(w, dec, [EC.long_prompt(505), EC.long_prompt(761)], 16, allow=EC.FORCED_ALLOW)
    assert finish == ["max_new_tokens"] * 2
    for b, case in enumerate(("cross_512", "cross_768")):
        assert ids[b].tolist() == EC.long_sequence(case)[0][EC.LONG_CASES[case]["plen"]:].tolist()


# ---- more than 17 rows --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [33, 48, 49, 64])
def test_many_rows_gemm_prefill(B):
    w, dec = model("uniform", block=128)
    lengths = seeded_lengths(B)
    assert sum(lengths) > 64
    ids, finish = run(w, dec, prompts_of(lengths, V_SMALL), 3)
    assert finish == ["max_new_tokens"] * B and len({tuple(i.tolist()) for i in ids}) > B // 2


def test_64_rows_linear_prefill():
    w, dec = model("peaky", block=128)
    _, finish = run(w, dec, prompts_of([1] * 64, V_SMALL), 3)
    assert finish == ["max_new_tokens"] * 64


# ---- how rows end ---------------------------------------------------------------------------------------------------------------------------------
def test_a_row_born_finished_beside_a_running_one():
    w, dec = model("uniform", block=128)
    prompts = prompts_of([128, 5], V_SMALL)
    u = seeded_uniforms(SEED, 2, 4)
    ids, finish, logits = dec.generate(prompts, 4, 0.8, 100, -1, uniforms=u, return_logits=True)
    assert finish == ["block_size", "max_new_tokens"]
    assert len(ids[0]) == 0 and logits[0].shape == (0, V_SMALL) and bool((dec.last_raw_ids[0] == -1).all())
    dec.last_raw_ids = dec.last_raw_ids[1:]      # verify_generation reads the raw buffer by row
    verify_generation(w, dec, prompts[1:], ids[1:], finish[1:], logits[1:], u[1:], 0.8, 100, -1, 4)


@pytest.mark.parametrize("max_new", [16, 17, 40])
def test_every_row_stops(small_first, max_new):
    """Step 1 may produce the stop token only: every row is finished long before max_new, at the host's check after 16 steps (17, 40) or never looked at
    (16). The next call on the same decoder must not see what this one left."""
    w, dec = model("uniform", block=128)
    stop = 1234
    prompts = prompts_of([4, 9, 2], V_SMALL, seed=11)
    ids, finish, logits = checked(w, dec, prompts, max_new, stop_token=stop, allow=[[0, V_SMALL, 0, 0], [stop, stop + 1, 0, 0]])
    assert finish == ["stop"] * 3 and [len(i) for i in ids] == [1] * 3 and [l.shape[0] for l in logits] == [2] * 3
    assert same(small_prefill(), small_first)
    ids, finish, logits = checked(w, dec, prompts, max_new, stop_token=stop, allow=[[stop, stop + 1, 0, 0], [stop, stop + 1, 0, 0]])
    assert finish == ["stop"] * 3 and [len(i) for i in ids] == [0] * 3 and [l.shape[0] for l in logits] == [1] * 3
    assert same(small_prefill(), small_first)


@pytest.mark.parametrize("bad", [V_SMALL, -1])
def test_id_outside_the_vocabulary(small_first, bad):
    _, dec = model("uniform", block=128)
    prompts = prompts_of(SMALL, V_SMALL)
    prompts[2][5] = bad
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        dec.generate(prompts, 4, uniforms=seeded_uniforms(SEED, 4, 4))
    assert same(small_prefill(), small_first)


def test_prompt_padding_is_not_read():
    _, dec = model("uniform", block=128)
    lib = dec.lib
    B, P, max_new = 2, 8, 4
    u = torch.full((B, max_new), 0.5, device=DEV)
    nbytes = lib.at_gpt_state_bytes(dec.handle, B, P + max_new)
    results = []
    for pad in (0, 1 << 30):
        host = np.random.default_rng(5).integers(0, V_SMALL, size=(B, P)).astype(np.int32)
        host[1, 3:] = pad
        prompts = torch.from_numpy(host).to(DEV)
        out = torch.full((B, max_new), -1, dtype=torch.int32, device=DEV)
        n = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        fin = torch.full((B,), -7, dtype=torch.int32, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        state = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
        rc = lib.at_gpt_generate(dec.handle, prompts.data_ptr(), P, (C.c_int32 * B)(P, 3), B, max_new, 0.8, 100, -1, u.data_ptr(), None, out.data_ptr(),
                                 n.data_ptr(), fin.data_ptr(), None, state.data_ptr(), nbytes, P + max_new, _cabi.current_stream_handle(DEV), status.data_ptr())
        assert rc == 0, _cabi.last_error()
        torch.cuda.synchronize()
        assert int(status) == 0, "the padding is not an id"
        results.append((out.cpu(), n.tolist(), fin.tolist()))
    (ids0, n0, fin0), (ids1, n1, fin1) = results
    assert n0 == n1 == [max_new] * B and fin0 == fin1 == [2] * B and torch.equal(ids0, ids1)


def test_state_buffer_reused_across_shapes():
    """X (3 rows, contexts of several hundred keys), Y (64 short rows: another carving of the same buffer), X again: what the buffer held does not matter."""
    w, dec = model("peaky")
    x_prompts = [EC.long_prompt(505), prompts_of([300], V_SMALL)[0], prompts_of([10], V_SMALL)[0]]
    first = checked(w, dec, x_prompts, 8)
    _, finish = run(w, dec, prompts_of(seeded_lengths(64), V_SMALL), 3)
    assert finish == ["max_new_tokens"] * 64
    u = seeded_uniforms(SEED, 3, 8)
    again = dec.generate(x_prompts, 8, 0.8, 100, -1, uniforms=u, return_logits=True)
    assert same(again, first)


# ---- the sampler alone: widths ------------------------------------------------------------------------------------------------------------------
def mid_step_draws(z, temperature, top_k, allow=None):
    """One draw per row at the middle of a kept id's CDF step, the r-th most probable id for row r (mod 3): as far from the step's two boundaries as the
    row allows. ``sampler_case`` then checks its precondition on them."""
    u = []
    for r in range(z.shape[0]):
        kept, p = R.kept_weights(z[r], temperature, top_k, allow)
        order = np.argsort(p, kind="stable")
        j = int(order[-1 - min(r % 3, kept.size - 1)])
        if p[j] < 1e-3:     # a step too narrow to stand 1e-4 from its ends: the widest one
            j = int(order[-1])
        cdf = np.cumsum(p)
        u.append((cdf[j] - 0.5 * p[j]))
    return np.array(u, dtype=np.float32)


@pytest.mark.parametrize("V", [1, 2, 63, 64, 65, 1000, 1023, 1025, 65536])
def test_sampler_widths(V):
    z = spread_logits(3, V, seed=V)
    for top_k in (1, 100, V, V + 5):
        for temperature in (0.8, 1.0):
            sampler_case(z, temperature, top_k, mid_step_draws(z, temperature, top_k))
    # all-equal logits, every id kept: the CDF is a ramp of V equal steps, and the last lanes of the walk's last group lie past the end
    if V <= 1025:
        t = np.zeros((3, V), dtype=np.float32)
        sampler_case(t, 1.0, V, [(j + 0.5) / V for j in (0, V // 2, V - 1)])


def test_sampler_many_rows():
    z = spread_logits(300, 1000, seed=300)
    sampler_case(z, 0.8, 100, mid_step_draws(z, 0.8, 100))


# ---- the sampler alone: rows whose threshold the last radix passes decide --------------------------------------------------------------------------
def radix_rows():
    """name -> one row. The first two differ in the low 10 bits of the mantissa only (one exponent), so the first two 8-bit passes of the radix select see
    one bin and the last two decide; the third mixes both zeros, denormals of both signs and the smallest normals: keys that differ in the sign bit and the
    low bits."""
    V = 1000
    perm = np.random.default_rng(23).permutation(V).astype(np.float32)
    near_one = (1.0 + perm * 2.0 ** -23).astype(np.float32)
    assert np.unique(near_one).size == V
    tiny = np.float32(2.0 ** -149)
    k = np.arange(1, 61, dtype=np.float32)
    normal = (np.float32(2.0 ** -126) * (1.0 + np.arange(61, dtype=np.float32) * np.float32(2.0 ** -23))).astype(np.float32)
    mixed = np.concatenate([[np.float32(0.0), np.float32(-0.0)], k * tiny, -(k * tiny), normal, -normal]).astype(np.float32)
    assert np.unique(mixed).size == mixed.size - 1 and int(np.signbit(mixed[mixed == 0]).sum()) == 1, "distinct but for the two zeros"
    mixed = mixed[np.random.default_rng(24).permutation(mixed.size)]
    return {"near_one": near_one, "near_minus_one": -near_one, "zeros_denormals": mixed}


@pytest.mark.parametrize("name", ["near_one", "near_minus_one", "zeros_denormals"])
def test_sampler_low_radix_passes(name):
    row = radix_rows()[name]
    top_ks = [1, 7, 100] + ([122] if name == "zeros_denormals" else [])   # 121 positive values: the 122nd largest is a zero, and both zeros stay
    for top_k in top_ks:
        kept, p = R.kept_weights(row, 1.0, top_k)
        assert kept.size == (123 if top_k == 122 else top_k)
        if top_k == 122:
            assert {int(i) for i in np.nonzero(row == 0)[0]} <= set(kept.tolist())
        js = sorted({0, kept.size // 2, kept.size - 1})
        z = np.stack([row] * len(js))
        sampler_case(z, 1.0, top_k, [(j + 0.5) / kept.size for j in js])   # weights equal to 1 within 2^-13: the middle of the j-th of kept equal steps


# ---- the fallback never returns an id of weight zero ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", [65, 1000])
def test_fallback_is_the_highest_finite_id(V):
    """u = 1 and kept weights that are all 1 (a power of two: every fp32 sum is exact in any order), so no running sum exceeds u S and the fallback
    decides; with top_k >= V the threshold is -inf and every id is kept, the -inf ones too, which the fallback must pass over."""
    u = torch.ones(2, device=DEV)
    zeros = np.zeros((2, V), dtype=np.float32)
    trailing = zeros.copy()
    trailing[0, V // 2:] = -np.inf
    trailing[1, 1:] = -np.inf
    for z, allow, want in ((zeros, (2, 10, 0, 0), [9, 9]), (zeros, (0, 1, 3, V - 1), [V - 2, V - 2]), (trailing, None, [V // 2 - 1, 0]), (zeros, None, [V - 1, V - 1])):
        for top_k in (V, V + 5):
            assert [R.sample(z[b], 1.0, top_k, 1.0, allow)[0] for b in range(2)] == want
            assert topk_sample(torch.from_numpy(z).to(DEV), 1.0, top_k, u, allow).cpu().tolist() == want


def test_fallback_through_generate():
    """Allow ranges of one id (one weight, 1, and zeros: every sum is exact) and u = 1: no running sum exceeds u S, so every step falls back, to the
    allowed id and not to id V - 1, whose weight is zero."""
    w, dec = model("uniform", block=128)
    allow = [[8, 9, 0, 0], [0, 0, 42, 43]]
    ids, finish, _ = checked(w, dec, prompts_of([6, 2], V_SMALL), 4, temperature=1.0, top_k=V_SMALL, allow=allow, uniforms=np.ones((2, 4), dtype=np.float32))
    assert finish == ["max_new_tokens"] * 2 and [i.tolist() for i in ids] == [[8, 42, 8, 42]] * 2
