"""GPU: the long form of semantic-to-acoustic generation (csrc/gpt.hip: at_gpt_generate_long) against the CPU twin in tests/gpt_ref.py.

The protocol is tests/test_semantic_decoder_gpu.py's, applied per window (``verify_long``): the prompt of window k is rebuilt from the DEVICE's own stream
(source ids + the offset, INFER, the carried ids); the twin runs once per window, teacher-forced on that prompt and the window's ids. (a) every device
logit vector is within ``parity.FLOAT_TOL`` of the twin's float64 logits; (b) the device's id equals ``gpt_ref.sample`` applied to the DEVICE's logits with
the draw at that stream position and that window's allow set, waived only where the draw lies within 2 (kept 2^-24 + 2^-22) of a CDF boundary, for at
most 2 % of a test's steps; (c) a non-final window has its exact count, the final one ends as the finish rules say, and nothing is written past a row's
length. tests/test_long_form_cpu.py shows on the twin alone that these inputs do not lean on the waiver and that a lost or shifted carry cannot pass (a)."""
import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.configs import Tokenizers, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, acoustic_windows, seeded_uniforms

from tests import gpt_ref as R
from tests import long_form_cases as K
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_decoders = {}


def window(kept):
    return 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)


def decoder(family, block=K.BLOCK, cfg=K.CFG):
    key = (family, block, cfg.max_source_tokens)
    if key not in _decoders:
        w = K.weights(family, block)
        _decoders[key] = (w, SemanticToAcoustic(cfg, device=DEV, weights=w))
    return _decoders[key]


def verify_long(w, dec, cfg, srcs, out, u, S, H, max_new, r=K.r, temperature=K.TEMPERATURE, top_k=K.TOP_K):
    block, raw = dec.block_size, dec.last_raw_ids
    waived = steps = 0
    worst = 0.0
    for b, src in enumerate(srcs):
        plan = acoustic_windows(len(src), S, H, r, block)
        stream = (out.ids[b] + cfg.ACOUSTIC_OFFSET).numpy()
        n, L, stopped = len(stream), out.logits[b].numpy(), out.finish[b] == "stop"
        # (c) structure
        assert L.shape[0] == n + (1 if stopped else 0)
        assert cfg.STOP_TOKEN not in stream.tolist(), "the stop token is not emitted"
        assert np.array_equal(raw[b, :n].numpy(), stream) and bool((raw[b, n:] == -1).all()), "nothing is written past a row's length"
        assert out.windows[b][:-1] == plan[:-1] and out.windows[b][-1][:3] == plan[-1][:3], "windows is the schedule"
        assert out.codes[b] is not None and out.codes[b].shape == (2, n // 2), "every id lies in the code book of its parity"
        for k, win in enumerate(plan):
            final = k == len(plan) - 1
            prompt, base = K.window_prompt(cfg, src, stream, win, r)
            P = len(prompt)
            if final:
                new, budget = n - base, min(max_new, block - P)
                assert new >= 0 and out.windows[b][-1][3] == new
                if stopped:
                    assert new < budget and new % 2 == 0, "STOP only on even steps"
                elif out.finish[b] == "max_new_tokens":
                    assert new == max_new and P + new <= block
                else:
                    assert out.finish[b] == "block_size" and P + new == block and new < max_new
                rows = new + (1 if stopped else 0)
            else:
                new = rows = win[3]
                assert n >= base + new, "a non-final window produces its exact count"
            ids_k = stream[base:base + new]
            Lk = L[base:base + rows]
            # (a) the float bar, teacher-forced on the device's own prompt and ids
            ref = R.forward(w, np.concatenate([prompt, ids_k]), torch.float64, positions=list(range(P - 1, P - 1 + rows))).numpy()
            diff = float(np.abs(Lk.astype(np.float64) - ref).max())
            worst = max(worst, diff)
            assert diff <= FLOAT_TOL, f"row {b} window {k}: logits differ from the float64 twin by {diff:.3e}"
            # (b) the sampler, exactly, on the device's logits
            allow = K.allow_of(cfg, final)
            for s in range(rows):
                want = int(ids_k[s]) if s < new else cfg.STOP_TOKEN
                tok, dist, kept = R.sample(Lk[s], temperature, top_k, u[b, base + s], allow[s % 2])
                steps += 1
                if tok != want:
                    assert dist < window(kept), (f"row {b} window {k} step {s}: device token {want}, rule gives {tok}, {dist:.3e} from a boundary "
                                                 f"(window {window(kept):.3e})")
                    waived += 1
    print(f"largest logit difference {worst:.3e}; waived {waived} of {steps} steps")
    assert waived <= 0.02 * steps
    return worst, waived


def run_long(w, dec, cfg, srcs, S, H, max_new, u=None, **geometry):
    if u is None:
        u = K.draws([len(s) for s in srcs], max_new, S=S, H=H, block=dec.block_size, **geometry)
    out = dec.to_acoustic_long(srcs, window=S, hop=H, max_new_tokens=max_new, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True)
    verify_long(w, dec, cfg, srcs, out, u, S, H, max_new)
    return out, u


def by_hand(dec, cfg, src, u_row, S, H, max_new, r=K.r):
    """The same windows through existing ``generate`` calls, the prompt rebuilt on the host every time."""
    plan = acoustic_windows(len(src), S, H, r, dec.block_size)
    stream, logits, finish = [], [], None
    for k, win in enumerate(plan):
        final = k == len(plan) - 1
        prompt, base = K.window_prompt(cfg, src, stream, win, r)
        n_new = max_new if final else win[3]
        ids, fin, lg = dec.generate([prompt.astype(np.int32)], n_new, K.TEMPERATURE, K.TOP_K, cfg.STOP_TOKEN if final else -1,
                                    uniforms=u_row[None, base:base + n_new], allow=K.allow_of(cfg, final), return_logits=True)
        assert final or (fin[0] == "max_new_tokens" and len(ids[0]) == n_new)
        stream += ids[0].tolist()
        logits.append(lg[0])
        finish = fin[0]
    return torch.tensor(stream, dtype=torch.int64), finish, torch.cat(logits)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("N", K.LENGTHS)
def test_one_row_follows_the_protocol_and_equals_the_by_hand_chain(family, N):
    w, dec = decoder(family)
    src = K.source(N)
    out, u = run_long(w, dec, K.CFG, [src], K.S, K.H, K.MAX_NEW)
    assert len(out.windows[0]) == (1 if N <= K.S else -(-(N - K.S) // K.H) + 1)
    ids, finish, logits = by_hand(dec, K.CFG, src, u[0], K.S, K.H, K.MAX_NEW)
    assert torch.equal(out.ids[0] + K.CFG.ACOUSTIC_OFFSET, ids) and out.finish[0] == finish, "id for id the chain of generate calls"
    assert torch.equal(out.logits[0], logits), "logit for logit: a single row takes the same prefill route and step kernel"


@pytest.mark.parametrize("max_new", [K.MAX_NEW, 1024])
def test_short_sources_equal_to_acoustic(max_new):
    """N <= S: what ``to_acoustic(constrain=True)`` gives with the same uniforms; at 1024 the rows run into the block (64 positions) as they do there."""
    w, dec = decoder("uniform")
    srcs = [K.source(N, seed=1) for N in (1, K.S - 1, K.S)]
    u = seeded_uniforms(K.SEED, len(srcs), max_new)
    want = dec.to_acoustic(srcs, max_new_tokens=max_new, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, constrain=True, return_logits=True)
    got = dec.to_acoustic_long(srcs, max_new_tokens=max_new, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True)   # the default window: (8, 4)
    assert got.finish == want.finish and (max_new != 1024 or "block_size" in got.finish)
    for b in range(len(srcs)):
        assert torch.equal(got.ids[b], want.ids[b]) and torch.equal(got.logits[b], want.logits[b]) and torch.equal(got.codes[b], want.codes[b])
        assert got.windows[b] == [(0, len(srcs[b]), 0, len(got.ids[b]))]
    assert want.windows is None


def test_rows_of_one_to_four_windows_share_their_passes():
    """S = 16, H = 8 at a block of 128: rows of 1, 16, 17 and 35 ids have 1, 1, 2 and 4 windows. Pass 0 prefills 2 + 17 + 17 + 17 = 53 tokens (the step kernel's
    route), pass 1 the final window of the third row beside a non-final one of the fourth, 34 + 41 = 75 tokens (the GEMM's route)."""
    S, H = 16, 8
    w, dec = decoder("peaky", block=128)
    srcs = [K.source(N, seed=2) for N in (1, S, S + 1, 2 * S + 3)]
    out, _ = run_long(w, dec, K.CFG, srcs, S, H, K.MAX_NEW)
    assert [len(x) for x in out.windows] == [1, 1, 2, 4]
    plans = [acoustic_windows(len(s), S, H, K.r, 128) for s in srcs]
    tokens = [sum(p[k][1] + 1 + p[k][2] for p in plans if len(p) > k) for k in range(4)]
    assert tokens == [53, 75, 41, 36] and max(tokens) > 64 >= min(tokens), "both prefill routes run"
    for b, plan in enumerate(plans):
        assert out.windows[b][:-1] == plan[:-1] and out.windows[b][-1][:3] == plan[-1][:3]


def test_stop_is_refused_inside_a_stream_and_taken_at_its_end():
    """The STOP row of ``wte`` scaled by 30: STOP leads the logits at many steps. Non-final windows still produce their exact count, the final windows stop,
    and each row is what it is when run alone."""
    base_w = K.weights("peaky")
    wte = base_w["transformer.wte.weight"].copy()
    wte[K.CFG.STOP_TOKEN] *= 30.0
    w = {**base_w, "transformer.wte.weight": wte}
    dec = SemanticToAcoustic(K.CFG, device=DEV, weights=w)
    srcs = [K.source(N, seed=4) for N in (K.S - 1, K.S + 1, 2 * K.S + 3)]
    out, u = run_long(w, dec, K.CFG, srcs, K.S, K.H, K.MAX_NEW)
    assert out.finish == ["stop"] * 3
    for b in (1, 2):
        start, _, carry, new = out.windows[b][-1]
        first_final = K.r * start + carry
        assert len(out.ids[b]) == first_final + new >= first_final, "every non-final window produced its exact count"
        leads = out.logits[b][:first_final:2].argmax(-1) == K.CFG.STOP_TOKEN
        assert int(leads.sum()) >= 1, "STOP led the logits at an even step of a non-final window and was refused"
    for b, src in enumerate(srcs):
        alone = dec.to_acoustic_long([src], window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u[b:b + 1])
        assert torch.equal(alone.ids[0], out.ids[b]) and alone.finish[0] == out.finish[b], "the other rows do not disturb a row"


def test_sixty_four_rows_twice_in_one_state():
    w, dec = decoder("uniform")
    lengths = [1 + (7 * i) % (2 * K.S + 3) for i in range(64)]
    srcs = [K.source(N, seed=5 + i) for i, N in enumerate(lengths)]
    u = K.draws(lengths, K.MAX_NEW)
    kw = dict(window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u)
    a = dec.to_acoustic_long(srcs, **kw)
    raw = dec.last_raw_ids.clone()
    b = dec.to_acoustic_long(srcs, **kw)
    assert a.finish == b.finish and all(torch.equal(x, y) for x, y in zip(a.ids, b.ids)), "the same call twice gives the same ids"
    assert torch.equal(raw, dec.last_raw_ids)
    assert len({len(x) for x in a.windows}) == 4, "rows of 1 to 4 windows"
    for i, ids in enumerate(a.ids):
        n = len(ids)
        start, _, carry, new = a.windows[i][-1]
        assert n == K.r * start + carry + new and (a.finish[i] != "max_new_tokens" or new == K.MAX_NEW)
        assert bool((raw[i, :n] == ids + K.CFG.ACOUSTIC_OFFSET).all()) and bool((raw[i, n:] == -1).all()), "nothing is written past a row's length"
        assert a.codes[i] is not None


def test_product_geometry():
    """S = 250, H = 124 at a block of 1024, N = S + H + 1: three windows whose contexts reach 1001 keys (two full non-final windows of 251 and 629 prompt
    tokens with 750 and 372 new ids)."""
    S, H = 250, 124
    w, dec = decoder("peaky", block=1024, cfg=K.CFG_PRODUCT)
    src = K.source(S + H + 1, seed=6, cfg=K.CFG_PRODUCT)
    out, _ = run_long(w, dec, K.CFG_PRODUCT, [src], S, H, 16)
    assert [x[:3] for x in out.windows[0]] == [(0, 250, 0), (124, 250, 378), (248, 127, 378)]
    assert [x[3] for x in out.windows[0][:2]] == [750, 372] and len(out.ids[0]) == 1122 + out.windows[0][2][3]


def test_to_audio_long_form_is_the_three_stages_composed():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.fine_decoder import seeded_uniforms as fine_uniforms
    from tests import fine_cases, fine_ref
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    fine_w = fine_cases.weights("a", "peaky")
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_w)
    tokens = (np.arange(13) * 7) % 1000      # 3 windows at (8, 4)
    kw = dict(long_form=True, window=8, hop=4, max_new_tokens=20)
    u1 = seeded_uniforms(11, 1, 36 + 20)
    coarse_by_hand = sem.to_acoustic(tokens, uniforms=u1, **kw)
    assert len(coarse_by_hand.windows[0]) == 3 and [x[3] for x in coarse_by_hand.windows[0][:2]] == [24, 12]
    T = coarse_by_hand.codes[0].shape[1]
    assert 18 <= T <= 28, "36 ids before the final window, at most 20 in it"
    u2 = fine_uniforms(12, 1, len(fine_ref.fine_windows(T, 128)), 128)
    fine_by_hand = sem.to_fine(coarse_by_hand.codes, uniforms=u2)
    audio, coarse, fine = sem.to_audio(tokens, uniforms=u1, fine_uniforms=u2, **kw)
    assert torch.equal(coarse.ids[0], coarse_by_hand.ids[0]) and coarse.windows == coarse_by_hand.windows
    assert torch.equal(fine.codes[0], fine_by_hand.codes[0]) and torch.equal(fine.codes[0][:2], coarse.codes[0])
    want = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8).decode(fine_by_hand.codes[0].unsqueeze(0))
    assert audio[0].shape == (1, 320 * T) and audio[0].dtype == torch.float32 and bool(torch.isfinite(audio[0]).all())
    assert torch.equal(audio[0], want), "to_audio(long_form=True) is bit-equal to the three stages composed by hand"
    short = sem.to_acoustic(tokens, max_new_tokens=20, uniforms=u1[:, :20], constrain=True)
    assert short.windows is None and len(short.ids[0]) <= 20, "without long_form nothing changes"


def test_refusals_raise_before_any_launch():
    from audiotoken_amd import AudioToken
    w, dec = decoder("uniform")
    good = K.source(2 * K.S + 3)
    u = K.draws([len(good)], K.MAX_NEW)
    before = dec.to_acoustic_long([good], window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, uniforms=u)
    raw = dec.last_raw_ids
    status = dec._status.clone()
    for kw, src in [(dict(window=7), good), (dict(hop=3), good), (dict(hop=10), good), (dict(window=16, hop=8), good),    # 16 + 1 + 48 > 64
                    (dict(), np.zeros(0, dtype=np.int64)), (dict(), np.array([K.CFG.SEMANTIC_VOCAB_SIZE])), (dict(), np.array([-1])),
                    (dict(), [good] * 65), (dict(), []), (dict(), np.zeros(65537, dtype=np.int64)), (dict(max_new_tokens=0), good),
                    (dict(max_new_tokens=1025), good), (dict(uniforms=u[:, :5]), good), (dict(uniforms=np.zeros((2, 100), dtype=np.float32)), good)]:
        with pytest.raises(ValueError):
            dec.to_acoustic_long(src, **{**dict(window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW), **kw})
        assert dec.last_raw_ids is raw and torch.equal(dec._status, status), "a refused call reaches neither the library nor the device"
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=w)
    for kw in (dict(window=8), dict(hop=4)):
        with pytest.raises(ValueError, match="long_form"):
            sem.to_acoustic(good, **kw)
        with pytest.raises(ValueError, match="long_form"):
            sem.to_audio(good, **kw)
    assert getattr(sem, "semantic_decoder", None) is None, "refused before a model is built"
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device=DEV).to_acoustic(good, long_form=True)
    again = dec.to_acoustic_long([good], window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, uniforms=u)
    assert torch.equal(again.ids[0], before.ids[0])
