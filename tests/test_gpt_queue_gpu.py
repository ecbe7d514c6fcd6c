"""GPU: the generation queue (csrc/gpt.hip: at_gpt_generate_queue): any number of sources through ``slots`` cache rows, each source
following §19's schedule on its own. The protocol is tests/test_long_form_gpu.py's ``verify_long``, imported and applied per source: the result's rows are
the sources, so (a) the float bar against the float64 twin, (b) the sampler on the device's own logits with the draw of that stream position, waived only
within 2 (kept 2^-24 + 2^-22) of a CDF boundary for at most 2 % of a test's steps, and (c) the structure hold whatever slot and tick a window ran in.
tests/test_gpt_queue_cpu.py shows on the twin alone that these inputs (tests/gpt_queue_cases.py) do not lean on the waiver, and checks the scheduler."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.configs import Tokenizers, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import (DEFAULT_TICK_WINDOWS, AcousticGeneration, SemanticToAcoustic, acoustic_windows, queue_tick_bound, queue_ticks, seeded_uniforms,
                                             window_steps)

from tests import gpt_queue_cases as Q
from tests import long_form_cases as K
from tests.test_long_form_gpu import DEV, decoder, verify_long

pytestmark = pytest.mark.gpu


def run_queue(dec, case, srcs, u, slots, tick_tokens=None, return_logits=True):
    return dec.to_acoustic_long(srcs, window=case["S"], hop=case["H"], max_new_tokens=case["max_new"], temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u,
                                return_logits=return_logits, slots=slots, tick_tokens=tick_tokens)


def verify(w, dec, cfg, case, srcs, out, u, rows=None):
    """``verify_long`` on the sources ``rows`` (default all) of a queue result."""
    if rows is None:
        return verify_long(w, dec, cfg, srcs, out, u, case["S"], case["H"], case["max_new"])
    pick = lambda xs: [xs[i] for i in rows]
    part = AcousticGeneration(ids=pick(out.ids), codes=pick(out.codes), finish=pick(out.finish), logits=pick(out.logits), windows=pick(out.windows))
    view = SimpleNamespace(block_size=dec.block_size, last_raw_ids=dec.last_raw_ids[rows])
    return verify_long(w, view, cfg, pick(srcs), part, u[rows], case["S"], case["H"], case["max_new"])


def check_trace(out, case, slots, tick_tokens, max_len):
    """The device's trace is the scheduler's, given the final windows' lengths the device produced; no tick is empty or exceeds ``tick_tokens``."""
    ticks, placement = queue_ticks(case["lens"], case["S"], case["H"], K.r, case["block"], case["max_new"], slots, tick_tokens, Q.final_steps(out))
    assert out.ticks == ticks and out.placement == placement
    assert all(1 <= a + c <= tick_tokens and route == (1 if a + c > 64 else 0) for a, _, c, route in out.ticks)
    assert len(out.ticks) <= queue_tick_bound(case["lens"], case["S"], case["H"], K.r, case["block"], case["max_new"])


def max_len_of(case):
    plans = [window_steps(acoustic_windows(N, case["S"], case["H"], K.r, case["block"]), case["max_new"], case["block"]) for N in case["lens"]]
    return max(P + n for plan in plans for P, n in plan)


@pytest.mark.parametrize("family", K.FAMILIES)
def test_one_slot_is_the_chain_of_one_row_calls(family):
    """``slots=1``: every tick is a lone prefill or a lone step on the routes a one-row call takes, so each source is bit-equal to ``to_acoustic_long([src])``
    with its row of the draws: ids, logits, finish, windows. Then a short source in the cache row a long one just used."""
    w, dec = decoder(family)
    for name in ("single", "reuse"):
        case = Q.CASES[name]
        srcs, u = Q.inputs(name)
        out = run_queue(dec, case, srcs, u, slots=1)
        assert [p[0] for p in out.placement] == [0] * len(srcs)
        assert all(a[2] < b[1] for a, b in zip(out.placement, out.placement[1:])), "one after the other"
        assert all(a + b == 1 for a, b, _, _ in out.ticks), "a lone prefill or a lone step"
        check_trace(out, case, 1, 1 + DEFAULT_TICK_WINDOWS * max_len_of(case), max_len_of(case))
        for i, src in enumerate(srcs):
            alone = dec.to_acoustic_long([src], window=case["S"], hop=case["H"], max_new_tokens=case["max_new"], temperature=K.TEMPERATURE, top_k=K.TOP_K,
                                         uniforms=u[i:i + 1], return_logits=True)
            assert torch.equal(out.ids[i], alone.ids[0]) and out.finish[i] == alone.finish[0] and out.windows[i] == alone.windows[0], (name, i)
            assert torch.equal(out.logits[i], alone.logits[0]), f"{name} source {i}: logit for logit"
            assert alone.ticks is None and alone.placement is None


@pytest.mark.parametrize("family", K.FAMILIES)
def test_four_slots_twelve_sources_mixed_ticks(family):
    w, dec = decoder(family)
    case = Q.CASES["mixed"]
    srcs, u = Q.inputs("mixed")
    out = run_queue(dec, case, srcs, u, slots=4)
    verify(w, dec, K.CFG, case, srcs, out, u)
    assert any(a > 0 and c > 0 for a, _, c, _ in out.ticks), "a tick with step tokens and prefill tokens together"
    used = [p[0] for p in out.placement]
    assert max(used.count(j) for j in range(4)) >= 2 and set(used) == {0, 1, 2, 3}, "a slot used by at least two sources"
    check_trace(out, case, 4, 4 + DEFAULT_TICK_WINDOWS * max_len_of(case), max_len_of(case))
    back = run_queue(dec, case, srcs[::-1], u[::-1].copy(), slots=4)
    verify(w, dec, K.CFG, case, srcs[::-1], back, u[::-1])


def test_both_routes_in_mixed_ticks():
    """S = 16, H = 8 at block 128 (prompts of 2 to 41 tokens), 8 slots, 18 sources of 1 to 4 windows. ``tick_tokens`` is the smallest ``slots + c max_len``
    at which the scheduler predicts a mixed tick on each route; the device's trace must show both and equal the scheduler's."""
    case = Q.CASES["routes"]
    w, dec = decoder("peaky", block=128)
    srcs, u = Q.inputs("routes")
    max_len = max_len_of(case)
    mixed = lambda ticks, route: [t for t in ticks if t[0] > 0 and t[2] > 0 and t[3] == route]
    for c in (1, 2, 4, 8):
        tick_tokens = 8 + c * max_len
        predicted, _ = queue_ticks(case["lens"], 16, 8, K.r, 128, case["max_new"], 8, tick_tokens)
        if mixed(predicted, 1) and mixed(predicted, 0):
            break
    else:
        raise AssertionError("no tick_tokens gives both routes")
    out = run_queue(dec, case, srcs, u, slots=8, tick_tokens=tick_tokens)
    assert {len(x) for x in out.windows} == {1, 2, 3, 4}
    big, small = mixed(out.ticks, 1), mixed(out.ticks, 0)
    assert big and all(a + c > 64 for a, _, c, _ in big), "a mixed tick of more than 64 tokens: the GEMM route and the scatter, with step tokens in it"
    assert small and all(a + c <= 64 for a, _, c, _ in small), "a mixed tick of at most 64 tokens"
    verify(w, dec, K.CFG, case, srcs, out, u)
    check_trace(out, case, 8, tick_tokens, max_len)


def test_tick_tokens_at_its_minimum():
    case = Q.CASES["mixed"]
    w, dec = decoder("peaky")
    srcs, u = Q.inputs("mixed")
    max_len = max_len_of(case)
    tick_tokens = 4 + max_len
    out = run_queue(dec, case, srcs, u, slots=4, tick_tokens=tick_tokens)
    verify(w, dec, K.CFG, case, srcs, out, u)
    check_trace(out, case, 4, tick_tokens, max_len)
    _, _, events = queue_ticks(case["lens"], case["S"], case["H"], K.r, case["block"], case["max_new"], 4, tick_tokens, Q.final_steps(out), detail=True)
    assert any(waiting for _, _, _, waiting in events), "windows wait: a slot with a window to begin has no token in some tick"
    roomy, _ = queue_ticks(case["lens"], case["S"], case["H"], K.r, case["block"], case["max_new"], 4, 4 + 8 * max_len, Q.final_steps(out))
    assert roomy != out.ticks
    assert max(a + c for a, _, c, _ in out.ticks) <= tick_tokens


def test_sixty_four_slots_130_sources_twice_in_one_state():
    case = Q.CASES["many"]
    w, dec = decoder("uniform")
    srcs, u = Q.inputs("many")
    a = run_queue(dec, case, srcs, u, slots=64)
    raw = dec.last_raw_ids.clone()
    verify(w, dec, K.CFG, case, srcs, a, u)          # every source, with logits
    b = run_queue(dec, case, srcs, u, slots=64, return_logits=False)
    assert a.finish == b.finish and all(torch.equal(x, y) for x, y in zip(a.ids, b.ids)), "the same call twice gives the same ids"
    assert torch.equal(raw, dec.last_raw_ids) and a.ticks == b.ticks and a.placement == b.placement
    for i, ids in enumerate(a.ids):
        n = len(ids)
        assert bool((raw[i, :n] == ids + K.CFG.ACOUSTIC_OFFSET).all()) and bool((raw[i, n:] == -1).all()), "nothing is written past a source's length"
    assert sorted({p[0] for p in a.placement}) == list(range(64))


def test_stop_heavy_sources_hand_their_slots_on_at_polls():
    case = Q.CASES["stop"]
    w = Q.stop_heavy_weights()
    dec = SemanticToAcoustic(K.CFG, device=DEV, weights=w)
    srcs, u = Q.inputs("stop")
    out = run_queue(dec, case, srcs, u, slots=2)
    verify(w, dec, K.CFG, case, srcs, out, u)        # non-final windows keep their exact counts
    assert out.finish == ["stop"] * len(srcs)
    assert any(win[-1][3] == 0 for win in out.windows), "a final window that stops at once"
    for win, ids in zip(out.windows, out.ids):
        start, _, carry, new = win[-1]
        assert len(ids) == K.r * start + carry + new
    check_trace(out, case, 2, 2 + DEFAULT_TICK_WINDOWS * max_len_of(case), max_len_of(case))
    budgets = [window_steps(acoustic_windows(N, case["S"], case["H"], K.r, case["block"]), case["max_new"], case["block"])[-1][1] for N in case["lens"]]
    early = [i for i, e in enumerate(Q.final_steps(out)) if e < budgets[i]]
    seen_at_poll = [i for i in early if (out.placement[i][2] + 1) % 16 == 0]
    assert seen_at_poll, "a source that stops inside its budget is seen at a poll (or, where none comes first, when its budget is used up)"
    by_slot = {}
    for p in sorted(out.placement, key=lambda p: p[1]):
        by_slot.setdefault(p[0], []).append(p)
    assert any(nxt[1] == prev[2] + 1 for row in by_slot.values() for prev, nxt in zip(row, row[1:])), "a slot is handed on at the tick after its poll"
    assert all(nxt[1] > prev[2] for row in by_slot.values() for prev, nxt in zip(row, row[1:])), "a slot never holds two sources"
    assert len(out.ticks) <= queue_tick_bound(case["lens"], case["S"], case["H"], K.r, case["block"], case["max_new"])


def test_product_geometry_with_a_prefill_beside_long_contexts():
    """S = 250, H = 124 at block 1024: sources of 375, 251 and 30 ids on two slots; the first source's contexts reach 1001 keys while the other slot prefills."""
    case = Q.PRODUCT
    w, dec = decoder("peaky", block=1024, cfg=K.CFG_PRODUCT)
    srcs, u = Q.inputs(case, cfg=K.CFG_PRODUCT)
    out = run_queue(dec, case, srcs, u, slots=2)
    verify(w, dec, K.CFG_PRODUCT, case, srcs, out, u)
    assert [len(x) for x in out.windows] == [3, 2, 1]
    assert [x[3] for x in out.windows[0][:2]] == [750, 372]
    assert out.placement[2][1] > out.placement[1][2] and out.placement[2][0] == 1, "the third source takes the second one's slot"
    assert any(a == 1 and c > 0 for a, _, c, _ in out.ticks), "a prefill beside a slot that steps over a long context"
    assert any(a == 0 and c > 64 for a, _, c, _ in out.ticks) and max(a + c for a, _, c, _ in out.ticks) > 1001


def test_to_audio_with_slots_is_the_three_stages_composed():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.fine_decoder import seeded_uniforms as fine_uniforms
    from tests import fine_cases
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))
    n_src = 70
    # 9 to 17 ids: 2 to 4 windows at (8, 4), so every source has at least the 24 ids = 12 frames of its first window (the acoustic decoder takes 7 frames or more)
    tokens = [(np.arange(9 + (5 * i) % 9) * 7 + i) % 1000 for i in range(n_src)]
    kw = dict(long_form=True, window=8, hop=4, max_new_tokens=12, slots=8)
    u1 = seeded_uniforms(21, n_src, 48 + 12)
    coarse = sem.to_acoustic(tokens, uniforms=u1, **kw)
    assert len(coarse.ids) == n_src and all(c is not None and c.shape[1] >= 1 for c in coarse.codes)
    u2 = fine_uniforms(22, n_src, 1, 128)                                             # every source has fewer than 128 frames: one fine window
    groups = [sem.to_fine(coarse.codes[:64], uniforms=u2[:64]), sem.to_fine(coarse.codes[64:], uniforms=u2[64:])]
    assert len(groups[1].codes) == 6
    by_hand = groups[0].codes + groups[1].codes
    audio, coarse2, fine = sem.to_audio(tokens, uniforms=u1, fine_uniforms=u2, **kw)
    assert all(torch.equal(a, b) for a, b in zip(coarse.ids, coarse2.ids)) and coarse2.placement == coarse.placement
    assert len(fine.codes) == n_src and all(torch.equal(a, b) for a, b in zip(fine.codes, by_hand))
    dec8 = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8)
    for i in range(n_src):
        want = dec8.decode(by_hand[i].unsqueeze(0))
        assert torch.equal(audio[i], want), f"source {i}: to_audio(long_form=True, slots=8) is bit-equal to the three stages composed by hand"


def test_refusals_raise_before_any_launch():
    from audiotoken_amd import AudioToken
    w, dec = decoder("uniform")
    good = K.source(2 * K.S + 3)
    u = K.draws([len(good)], K.MAX_NEW)
    base = dict(window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, slots=2)
    before = dec.to_acoustic_long([good], uniforms=u, **base)
    raw = dec.last_raw_ids
    status = dec._status.clone()
    max_len = K.S + 1 + K.r * K.S
    for kw, src in [(dict(slots=0), good), (dict(slots=65), good), (dict(), []), (dict(), [good[:1]] * 4097), (dict(tick_tokens=2 + max_len - 1), good),
                    (dict(tick_tokens=64 * 1025 + 1), good), (dict(uniforms=u[:, :5]), good), (dict(uniforms=np.zeros((2, 100), dtype=np.float32)), good),
                    (dict(slots=None, tick_tokens=100), good), (dict(window=7), good), (dict(max_new_tokens=0), good)]:
        with pytest.raises(ValueError):
            dec.to_acoustic_long(src, **{**base, **kw})
        assert dec.last_raw_ids is raw and torch.equal(dec._status, status), "a refused call reaches neither the library nor the device"
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=w)
    for kw in (dict(slots=4), dict(tick_tokens=100), dict(slots=4, tick_tokens=100)):
        with pytest.raises(ValueError, match="long_form"):
            sem.to_acoustic(good, **kw)
        with pytest.raises(ValueError, match="long_form"):
            sem.to_audio(good, **kw)
    assert getattr(sem, "semantic_decoder", None) is None, "refused before a model is built"
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device=DEV).to_acoustic(good, long_form=True, slots=4)
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device=DEV).to_audio(good, long_form=True, slots=4)
    again = dec.to_acoustic_long([good], uniforms=u, **base)
    assert torch.equal(again.ids[0], before.ids[0]) and again.placement == [(0, 0, again.placement[0][2])]
