"""GPU: teacher-forced scoring (csrc/gpt_score.hip: gpt_score_kernel, at_op_score_rows, at_gpt_score; semantic_decoder.py: score_rows, score_acoustic;
DESIGN.md §23) against the float64 twin in tests/gpt_score_ref.py, which tests/test_oracle_gpt_score_cpu.py pins to the reference's cross-entropy.

The bars. The op alone, on the same fp32 logits as the twin: ``rank`` exact, ``logprob`` within the derived ``logprob_bound`` (no waivers). The scorer
(``verify``): returned logits within ``parity.FLOAT_TOL`` of the twin's; ``logprob`` within ``2 FLOAT_TOL / T + bound`` of the twin's (the log-sum-exp is
1-Lipschitz in the sup norm and the target's logit moves by at most as much); ``rank`` between the twin's counts of ids above ``zt_t + 2 FLOAT_TOL / T``
and above ``zt_t - 2 FLOAT_TOL / T``; and, on the DEVICE's own returned logits, ``rank`` exactly numpy's count and ``logprob`` within the derived bound."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import weights as W
from audiotoken_amd.configs import Tokenizers, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, acoustic_stream, constrained_allow, score_logits

from tests import gpt_edge_cases as EC
from tests import gpt_ref as R
from tests import gpt_score_ref as SR
from tests import long_form_cases as K
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V_SMALL = 2048
FAMILIES = ["uniform", "peaky"]
RECORD = {"logit": 0.0, "logprob": 0.0, "logprob_on_device_logits": 0.0}
_models, _twin_logits = {}, {}


def model(family, block=1024, cfg=None):
    """(weights, decoder) of the 2-layer model with a 2048-id vocabulary."""
    key = (family, block, None if cfg is None else (cfg.max_source_tokens, cfg.STOP_TOKEN))
    if key not in _models:
        w = K.weights(family, block)
        _models[key] = (w, SemanticToAcoustic(cfg, device=DEV, weights=w))
    return _models[key]


def twin_logits(family, w, seq):
    """The twin's float64 logits at every position but the last of ``seq``, computed once per sequence."""
    key = (family, len(w["transformer.wpe.weight"]), np.asarray(seq, dtype=np.int64).tobytes())
    if key not in _twin_logits:
        _twin_logits[key] = R.forward(w, seq, torch.float64, positions=list(range(len(seq) - 1))).numpy()
    return _twin_logits[key]


# ---- the op alone ---------------------------------------------------------------------------------------------------------------------------------
def op_case(z, targets, temperature, allow=None):
    z = np.ascontiguousarray(z, dtype=np.float32)
    zd = torch.from_numpy(z).to(DEV)
    td = torch.tensor(list(targets), dtype=torch.int32, device=DEV)
    lp, rank = score_logits(zd, td, temperature, allow)
    lp2, rank2 = score_logits(zd, td, temperature, allow)
    assert torch.equal(lp.view(torch.int32), lp2.view(torch.int32)) and torch.equal(rank, rank2), "the same call twice gives equal bits"
    lp, rank = lp.cpu().numpy(), rank.cpu().numpy()
    worst = 0.0
    for b, t in enumerate(targets):
        want_lp, want_rank = SR.score(z[b], t, temperature, allow)
        assert rank[b] == want_rank, f"row {b}: rank {rank[b]}, the rule gives {want_rank}"
        if want_lp == -np.inf:
            assert lp[b] == -np.inf, f"row {b}: logprob {lp[b]}, the rule gives -inf"
            continue
        zt = SR.tempered(z[b], temperature, allow)
        bound = SR.logprob_bound(float(zt[t]) - float(zt.max()))
        err = abs(float(lp[b]) - want_lp)
        worst = max(worst, err / bound)
        assert err <= bound, f"row {b}: logprob {lp[b]!r} against {want_lp!r}: off by {err:.3e}, the derived bound is {bound:.3e}"
    return worst


def spread(R_, V, seed, scale=4.0):
    return (np.random.default_rng(seed).standard_normal((R_, V)) * scale).astype(np.float32)


WIDTHS = [1, 64, 1001, 2048, 53376, 65536]   # the issue's five, and an odd one: rows that start off a 16-byte boundary and end inside a group of four


@pytest.mark.parametrize("temperature", [1.0, 0.8, 0.05])
@pytest.mark.parametrize("V", WIDTHS)
def test_op_against_the_rule(V, temperature):
    z = spread(6, V, seed=V)
    rng = np.random.default_rng(V + 1)
    targets = [0, V - 1, int(z[2].argmax()), int(z[3].argmin())] + rng.integers(0, V, size=2).tolist()
    worst = op_case(z, targets, temperature)
    if V >= 64:
        allow = (V // 4, V // 2, V - 3, V - 2)
        worst = max(worst, op_case(z, [V // 4, V // 2 - 1, V - 3, V // 4 + 1, V // 3, V // 2 - 2], temperature, allow))
    print(f"V={V} T={temperature}: the largest |logprob - rule| is {worst:.2f} of the derived bound")


@pytest.mark.parametrize("temperature", [1.0, 0.8, 0.05])
@pytest.mark.parametrize("V", WIDTHS[1:])
def test_op_on_crafted_rows(V, temperature):
    z = spread(1, V, seed=3)[0]
    top = float(z.max())
    # ties at the target's value are not counted in rank: three ids share the target's value, two lie above
    t = z.copy(); t[[5, V // 4, V // 2, V - 1]] = top + 0.5; t[[7, V - 2]] = top + 1.0
    op_case(np.stack([t] * 4), [5, V // 2, V - 1, 7], temperature)
    # -inf entries; a target that is -inf itself; all but three ids -inf
    t = z.copy(); t[::2] = -np.inf
    op_case(np.stack([t, t]), [1, 2], temperature)
    t = np.full(V, -np.inf, dtype=np.float32); t[[3, V // 2, V - 1]] = [0.0, 1.0, 0.5]
    op_case(np.stack([t] * 3), [3, V // 2, V - 1], temperature)
    # all mass on one id: the rest -inf, and the rest so far below that their weights vanish
    t = np.full(V, -np.inf, dtype=np.float32); t[V // 3] = 2.5
    op_case(np.stack([t, t]), [V // 3, 0], temperature)
    t = np.full(V, -300.0, dtype=np.float32); t[V // 3] = 40.0
    op_case(np.stack([t, t]), [V // 3, 1], temperature)
    # logits spanning +/- 80: targets at the top, the bottom and between
    t = np.linspace(-80.0, 80.0, V).astype(np.float32)[np.random.default_rng(5).permutation(V)]
    op_case(np.stack([t] * 3), [int(t.argmax()), int(t.argmin()), V // 2], temperature)
    # a target outside the allow set; an allow range of width 1 (alone, and beside a wider one)
    op_case(np.stack([z] * 3), [V // 4 - 1, V // 2, V - 2], temperature, allow=(V // 4, V // 2, V - 3, V - 2))
    op_case(np.stack([z] * 2), [9, 10], temperature, allow=(9, 10, 0, 0))
    op_case(np.stack([z] * 2), [V - 3, V // 4], temperature, allow=(V // 4, V // 2, V - 3, V - 2))
    # a target that is not an id
    op_case(np.stack([z] * 2), [-1, V], temperature)


def test_op_on_a_single_id():
    for temperature in (1.0, 0.8, 0.05):
        op_case(np.array([[3.25], [-80.0], [0.0]], dtype=np.float32), [0, 0, 0], temperature)
        op_case(np.array([[3.25]], dtype=np.float32), [0], temperature, allow=(0, 1, 0, 0))


# ---- the scorer against the twin -----------------------------------------------------------------------------------------------------------------
def verify(family, w, seqs, froms, lp, rank, logits, temperature=1.0, allow=None):
    tol = 2 * FLOAT_TOL / temperature
    for b, (seq, first) in enumerate(zip(seqs, froms)):
        n = len(seq) - first
        assert lp[b].shape == (n,) and rank[b].shape == (n,) and logits[b].shape == (n, len(w["transformer.wte.weight"]))
        ref = twin_logits(family, w, seq)[first - 1:]
        L = logits[b].numpy()
        diff = float(np.abs(L.astype(np.float64) - ref).max())
        RECORD["logit"] = max(RECORD["logit"], diff)
        assert diff <= FLOAT_TOL, f"row {b}: logits differ from the float64 twin by {diff:.3e}"
        for j in range(n):
            a = None if allow is None else allow[j % 2]
            t = int(seq[first + j])
            got_lp, got_rank = float(lp[b][j]), int(rank[b][j])
            twin_row = ref[j].astype(np.float32)
            want_lp, _ = SR.score(twin_row, t, temperature, a)
            dev_lp, dev_rank = SR.score(L[j], t, temperature, a)
            assert got_rank == dev_rank, f"row {b} position {j}: rank {got_rank}, numpy counts {dev_rank} on the device's own logits"
            if want_lp == -np.inf:
                assert got_lp == -np.inf and got_rank == len(twin_row)
                continue
            zt = SR.tempered(twin_row, temperature, a).astype(np.float64)
            d = zt[t] - zt.max()
            err = abs(got_lp - want_lp)
            RECORD["logprob"] = max(RECORD["logprob"], err)
            assert err <= tol + SR.logprob_bound(d), f"row {b} position {j}: logprob {got_lp} against the twin's {want_lp}"
            assert int((zt > zt[t] + tol).sum()) <= got_rank <= int((zt > zt[t] - tol).sum()), f"row {b} position {j}: rank {got_rank}"
            zd = SR.tempered(L[j], temperature, a)
            err = abs(got_lp - dev_lp)
            RECORD["logprob_on_device_logits"] = max(RECORD["logprob_on_device_logits"], err)
            assert err <= SR.logprob_bound(float(zd[t]) - float(zd.max())), f"row {b} position {j}: {err:.3e} from the rule on the device's own logits"
    print(f"largest differences so far: logits {RECORD['logit']:.3e}, logprob {RECORD['logprob']:.3e} against the twin, "
          f"{RECORD['logprob_on_device_logits']:.3e} against the rule on the device's logits")


def run(family, seqs, froms, temperature=1.0, allow=None, block=1024, **passes):
    w, dec = model(family, block)
    lp, rank, logits = dec.score_rows(seqs, froms, temperature, allow, return_logits=True, **passes)
    verify(family, w, seqs, froms, lp, rank, logits, temperature, allow)
    raw_lp, raw_rank = dec.last_raw_scores
    for b, (seq, first) in enumerate(zip(seqs, froms)):
        n = len(seq) - first
        assert bool(torch.isnan(raw_lp[b, n:]).all()) and bool((raw_rank[b, n:] == -1).all()), "nothing is written past a row's count"
    return lp, rank, logits


def ids_of(L, seed):
    return np.random.default_rng(1000 * seed + L).integers(0, V_SMALL, size=L).astype(np.int32)


def same_bits(a, b):
    return all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(a[0], b[0])) and all(torch.equal(x, y) for x, y in zip(a[1], b[1]))


@pytest.mark.parametrize("family", FAMILIES)
def test_rows_of_every_length(family):
    """Lengths 2, 3, 64, 65, 257 and 1024 (the lost-key inputs of tests/gpt_edge_cases.py), each scored from 1, from the middle and from its last id."""
    seqs, froms = [], []
    for L in (2, 3, 64, 65, 257, 1024):
        seq = EC.long_sequence("longest")[0].astype(np.int32) if L == 1024 else ids_of(L, 1)
        assert len(seq) == L
        for first in sorted({1, max(1, L // 2), L - 1}):
            seqs.append(seq)
            froms.append(first)
    run(family, seqs, froms)


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("last", [43, 44])
def test_both_routes_of_the_prefill(family, last):
    """A call whose whole list is 64 tokens (the streaming linear kernel) and one of 65 (the GEMM), with a temperature and allow sets by parity. A row's
    last id is a target only, so a row of L ids puts L - 1 tokens into the list."""
    cfg = K.CFG
    rng = np.random.default_rng(last)
    seqs, froms = [], []
    for L in (2, 3, 20, last):
        first = max(1, L // 3)
        stream = [cfg.ACOUSTIC_OFFSET + cfg.codebook_size * (s % 2) + int(rng.integers(0, cfg.codebook_size)) for s in range(L - first)]
        if L == 20:
            stream[6] = cfg.STOP_TOKEN          # allowed on an even step,
            stream[9] = cfg.STOP_TOKEN          # not on an odd one
        seqs.append(np.array(rng.integers(0, V_SMALL, size=first).tolist() + stream, dtype=np.int32))
        froms.append(first)
    assert sum(len(s) - 1 for s in seqs) == 21 + last and 21 + last in (64, 65)
    lp, rank, _ = run(family, seqs, froms, temperature=0.8, allow=constrained_allow(cfg))
    assert float(lp[2][6]) > -np.inf and float(lp[2][9]) == -np.inf and int(rank[2][9]) == V_SMALL


def test_seventy_short_rows_make_two_passes():
    seqs = [ids_of(3 + b % 5, b) for b in range(70)]
    run("uniform", seqs, [1 + b % 2 for b in range(70)], rows=64)


def test_pass_tokens_splits_a_call_in_the_middle():
    seqs = [ids_of(40, b) for b in range(6)]
    split = run("peaky", seqs, [13] * 6, max_len=40, pass_tokens=100)     # two rows a pass
    whole = run("peaky", seqs, [13] * 6)
    for x, y in zip(split[0], whole[0]):
        assert float((x - y).abs().max()) <= SR.logprob_bound(0) + 2 * FLOAT_TOL


@pytest.mark.parametrize("scored", [30, 32, 33, 48])
def test_head_chunks(scored):
    """head_rows = 16 against a pass of 30, 32, 33 and 48 scored positions (the last chunk short, exactly full twice over, one position long, three full
    chunks), and head_rows = 4096: how the head is cut does not enter the results. The head cuts the PASS's scored positions: the two rows' together."""
    seqs, froms = [ids_of(60, 5), ids_of(60, 6)], [60 - (scored - 1), 59]
    assert sum(len(s) - f for s, f in zip(seqs, froms)) == scored
    small = run("uniform", seqs, froms, head_rows=16)
    large = run("uniform", seqs, froms, head_rows=4096)
    assert same_bits(small, large)


def test_state_reuse_across_calls():
    w, dec = model("peaky")
    a_seqs, a_from = [ids_of(257, 9), ids_of(70, 9)], [100, 1]
    first = run("peaky", a_seqs, a_from)
    run("peaky", [ids_of(5, 9)], [2])                     # a smaller call in the same workspace
    again = run("peaky", a_seqs, a_from)
    assert same_bits(first, again), "a call leaves nothing behind that the next one reads"


def test_an_id_outside_the_vocabulary_is_reported():
    w, dec = model("uniform")
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        dec.score_rows([np.array([1, 2, V_SMALL, 3], dtype=np.int32)], [1])
    with pytest.raises(ValueError, match="outside the model's vocabulary"):
        dec.score_rows([np.array([1, 2, 3, -1], dtype=np.int32)], [1])           # a row's last id is in no token list: reported as a target
    with pytest.raises(ValueError, match="1 to 65536 rows"):
        dec.score_rows([], [])


def test_argument_errors_launch_nothing():
    w, dec = model("uniform", block=64)
    lib = dec.lib
    n, L = 2, 8
    seq = torch.zeros((n, L), dtype=torch.int32, device=DEV)
    lp = torch.full((n, L), -7.0, device=DEV)
    rank = torch.full((n, L), -7, dtype=torch.int32, device=DEV)
    nbytes = lib.at_gpt_score_state_bytes(dec.handle, 2, L, 2 * L, 16)
    assert nbytes > 0
    state = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)

    def call(lens=(L, L), froms=(1, 1), n_rows=n, temperature=1.0, allow=None, state_ptr=state.data_ptr(), rows=2, max_len=L, pass_tokens=2 * L, head_rows=16,
             out_stride=L, nbytes=nbytes):
        c_allow = None if allow is None else (C.c_int32 * 8)(*allow)
        return lib.at_gpt_score(dec.handle, seq.data_ptr(), L, (C.c_int32 * len(lens))(*lens), (C.c_int32 * len(froms))(*froms), n_rows, temperature, c_allow,
                                lp.data_ptr(), rank.data_ptr(), out_stride, None, state_ptr, nbytes, rows, max_len, pass_tokens, head_rows,
                                _cabi.current_stream_handle(DEV), None)

    for kwargs, text in [(dict(n_rows=0), "n_rows"), (dict(n_rows=65537), "n_rows"), (dict(lens=(L, 1)), "seq_len of row 1"), (dict(lens=(L + 1, L)), "seq_len of row 0"),
                         (dict(froms=(0, 1)), "score_from of row 0"), (dict(froms=(1, L)), "score_from of row 1"), (dict(out_stride=L - 2), "out_stride"),
                         (dict(temperature=0.0), "temperature"), (dict(temperature=float("nan")), "temperature"), (dict(allow=[5, 4, 0, 0, 0, 1, 0, 0]), "allow ranges"),
                         (dict(rows=0), "rows must be"), (dict(rows=65), "rows must be"), (dict(max_len=65), "max_len"), (dict(max_len=1), "max_len"),
                         (dict(pass_tokens=L - 1), "pass_tokens"), (dict(head_rows=8), "head_rows"), (dict(head_rows=24), "head_rows"),
                         (dict(head_rows=4112), "head_rows"), (dict(state_ptr=None), "null state"), (dict(nbytes=nbytes - 1), "state too small")]:
        assert call(**kwargs) != 0, kwargs
        assert text in _cabi.last_error(), (kwargs, _cabi.last_error())
    assert lib.at_gpt_score_state_bytes(dec.handle, 0, L, 2 * L, 16) == 0 and lib.at_gpt_score_state_bytes(dec.handle, 2, L, L - 1, 16) == 0
    assert lib.at_gpt_score_state_bytes(dec.handle, 2, L, 2 * L, 20) == 0
    torch.cuda.synchronize()
    assert bool((lp == -7).all()) and bool((rank == -7).all()) and bool((state == 0).all()), "a refused call writes nothing"
    assert call() == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert bool((rank[:, :L - 1] >= 0).all()) and bool((rank[:, L - 1] == -7).all())


# ---- agreement with generation --------------------------------------------------------------------------------------------------------------------
def agrees_with_generator(out, score, cfg, temperature, allow, vocab):
    """Each scored logprob against the float64 rule applied to the generator's own recorded logits at the sampled id; STOP where the row stopped."""
    compared = 0
    for b in range(len(out.ids)):
        gen = out.logits[b].numpy()
        stream = (out.ids[b] + cfg.ACOUSTIC_OFFSET).tolist() + [cfg.STOP_TOKEN]
        assert gen.shape[0] == len(out.ids[b]) + (1 if out.finish[b] == "stop" else 0)
        assert score.logprob[b].shape == (len(out.ids[b]) + 1,)
        for s in range(gen.shape[0]):
            want, _ = SR.score(gen[s], stream[s], temperature, allow[s % 2])
            zt = SR.tempered(gen[s], temperature, allow[s % 2])
            bar = 2 * FLOAT_TOL / temperature + SR.logprob_bound(float(zt[stream[s]]) - float(zt.max()))
            got = float(score.logprob[b][s])
            assert want > -np.inf and abs(got - want) <= bar, f"source {b} position {s}: scored {got}, the rule on the generator's logits gives {want}"
            compared += 1
    return compared


@pytest.mark.parametrize("family", FAMILIES)
def test_scores_agree_with_the_logits_generation_drew_from(family):
    temperature = 0.8
    cfg = K.CFG_PRODUCT
    srcs = [K.source(n, cfg=cfg) for n in (5, 30, 60, 100)]
    generate = lambda dec: dec.to_acoustic(srcs, max_new_tokens=16, temperature=temperature, seed=K.SEED, constrain=True, return_logits=True)
    _, dec = model(family, cfg=cfg)
    out = generate(dec)
    if "stop" not in out.finish:
        # no row drew STOP: the id source 1 drew at step 6 becomes the STOP token of a second configuration, and with the same draws that source stops there
        cfg = dataclasses.replace(cfg, STOP_TOKEN=int(out.ids[1][6]) + cfg.ACOUSTIC_OFFSET)
        _, dec = model(family, cfg=cfg)
        out = generate(dec)
        assert out.finish[1] == "stop" and len(out.ids[1]) <= 6
    assert "stop" in out.finish and all(c is not None for c in out.codes)
    score = dec.score_acoustic(srcs, out.codes, temperature=temperature, constrain=True)
    n = agrees_with_generator(out, score, cfg, temperature, constrained_allow(cfg), V_SMALL)
    assert n >= sum(len(i) for i in out.ids) + 1
    for b in range(4):
        assert abs(score.nll[b] + float(score.logprob[b].double().mean())) < 1e-12 and score.rank[b].dtype == torch.int32


# ---- the long form --------------------------------------------------------------------------------------------------------------------------------
LONG_SOURCES = (8, 9, 21)


@pytest.mark.parametrize("family", FAMILIES)
def test_long_form_equals_score_rows_on_the_twin_s_rows(family):
    cfg = K.CFG
    w, dec = model(family, block=K.BLOCK, cfg=cfg)
    srcs = [K.source(N) for N in LONG_SOURCES]
    rng = np.random.default_rng(17)
    codes = [torch.from_numpy(rng.integers(0, cfg.codebook_size, size=(2, K.capacity(N, 6) // 2))) for N in LONG_SOURCES]
    score = dec.score_acoustic(srcs, codes, temperature=0.8, long_form=True, window=K.S, hop=K.H, return_logits=True)
    seqs, froms, owner = [], [], []
    for b, (src, c) in enumerate(zip(srcs, codes)):
        for seq, first, _ in SR.long_rows(src, acoustic_stream(c, cfg).tolist(), K.S, K.H, K.r, cfg.SEMANTIC_OFFSET, cfg.INFER_TOKEN, cfg.STOP_TOKEN):
            seqs.append(seq); froms.append(first); owner.append(b)
    assert [owner.count(b) for b in range(3)] == [1, 2, 5] and [len(w_) for w_ in score.windows] == [1, 2, 5]
    allow = constrained_allow(cfg)
    lp, rank, logits = run(family, seqs, froms, temperature=0.8, allow=allow, block=K.BLOCK)     # the twin's bars, on the twin's rows
    for b in range(3):
        mine = [i for i, o in enumerate(owner) if o == b]
        assert torch.equal(score.logprob[b].view(torch.int32), torch.cat([lp[i] for i in mine]).view(torch.int32)), "the same arithmetic: equal bits"
        assert torch.equal(score.rank[b], torch.cat([rank[i] for i in mine])) and torch.equal(score.logits[b], torch.cat([logits[i] for i in mine]))
        assert score.logprob[b].shape == (2 * codes[b].shape[1] + 1,)


@pytest.mark.parametrize("family", FAMILIES)
def test_long_form_agrees_with_long_form_generation(family):
    cfg = K.CFG
    w, dec = model(family, block=K.BLOCK, cfg=cfg)
    srcs = [K.source(N) for N in LONG_SOURCES]
    out = dec.to_acoustic_long(srcs, window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, seed=K.SEED, return_logits=True)
    assert all(c is not None for c in out.codes)
    score = dec.score_acoustic(srcs, out.codes, temperature=K.TEMPERATURE, long_form=True, window=K.S, hop=K.H)
    # What this shows: the scorer reproduces the generator's LOGITS at every stream position, carry and all. The rule applied to them is the scorer's
    # documented one: one pair of allow sets per call, STOP allowed on even positions of every window. Generation refuses STOP in non-final
    # windows, so there its own log-probs are higher by log1p of STOP's share; in the final window the two rules are the same.
    agrees_with_generator(out, score, cfg, K.TEMPERATURE, constrained_allow(cfg), K.V)
    assert [[w_[:3] for w_ in plan] for plan in score.windows] == [[w_[:3] for w_ in plan] for plan in out.windows]


# ---- the real row width ---------------------------------------------------------------------------------------------------------------------------
def test_real_vocabulary_through_the_public_interface():
    from audiotoken_amd import AudioToken
    cfg = Wav2VecBertDecoderConfig()
    w = W.synth_gpt_weights(n_layer=1, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=w)
    src = np.random.default_rng(5).integers(0, 1000, size=6)
    codes = torch.from_numpy(np.random.default_rng(6).integers(0, 1024, size=(2, 5)))
    for constrain, temperature in ((False, 1.0), (True, 0.8)):
        score = sem.score_acoustic(src, codes, temperature=temperature, constrain=constrain, return_logits=True)
        seq = np.concatenate([src + cfg.SEMANTIC_OFFSET, [cfg.INFER_TOKEN], acoustic_stream(codes, cfg), [cfg.STOP_TOKEN]])
        assert score.logprob[0].shape == (11,) and score.logits[0].shape == (11, cfg.VOCAB_SIZE) and score.windows is None
        verify("peaky53376", w, [seq], [7], score.logprob, score.rank, score.logits, temperature, constrained_allow(cfg) if constrain else None)
        assert np.isfinite(score.nll[0]) and abs(score.nll[0] + float(score.logprob[0].double().mean())) < 1e-12
