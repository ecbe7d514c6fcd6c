"""GPU: voice prompts in the GPT stage (csrc/gpt.hip: at_gpt_generate_long_prompted, at_gpt_generate_queue_prompted) against the CPU twin in
tests/gpt_ref.py.

The protocol is tests/test_long_form_gpu.py's (§17's, per window) on the concatenated source and stream of a prompted row (``verify``): the prompt of window
k is rebuilt from the prompt table and the DEVICE's own result; (a) every device logit vector is within ``parity.FLOAT_TOL`` of the twin's float64 logits;
(b) the device's id equals ``gpt_ref.sample`` on the DEVICE's logits with the draw at that RESULT position, waived only within 2 (kept 2^-24 + 2^-22) of a
CDF boundary, for at most 2 % of a test's steps; (c) the counts, the finish rules, and nothing written past a row's length. tests/test_gpt_prompt_cpu.py shows
on the twin alone that these inputs do not lean on the waiver and that a dropped or shifted prompt cannot pass (a). The self-carry identity is exact."""
import numpy as np
import pytest
import torch

from audiotoken_amd.semantic_decoder import SemanticToAcoustic, acoustic_windows
from audiotoken_amd.voice import VoicePrompt

from tests import gpt_ref as R
from tests import long_form_cases as K
from tests import voice_cases as VC
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


def verify(w, dec, cfg, srcs, voices, out, u, S, H, max_new, rows=None, r=K.r, temperature=K.TEMPERATURE, top_k=K.TOP_K):
    block, raw = dec.block_size, dec.last_raw_ids
    waived = steps = 0
    worst = 0.0
    for b in (range(len(srcs)) if rows is None else rows):
        src, vp = srcs[b], voices[b]
        P = 0 if vp is None else len(vp)
        off = r * P
        plan = acoustic_windows(len(src), S, H, r, block, P)
        result = (out.ids[b] + cfg.ACOUSTIC_OFFSET).numpy()
        C = VC.concatenated(vp, src)
        full = result if vp is None else np.concatenate([VC.given_stream(cfg, vp), result])
        n, L, stopped = len(result), out.logits[b].numpy(), out.finish[b] == "stop"
        assert L.shape[0] == n + (1 if stopped else 0)
        assert cfg.STOP_TOKEN not in result.tolist()
        assert np.array_equal(raw[b, :n].numpy(), result) and bool((raw[b, n:] == -1).all()), "the result excludes the prompt; nothing is written past its length"
        assert out.windows[b][:-1] == plan[:-1] and out.windows[b][-1][:3] == plan[-1][:3], "windows is the schedule of the concatenated source"
        assert out.codes[b] is not None and out.codes[b].shape == (2, n // 2)
        for k, win in enumerate(plan):
            final = k == len(plan) - 1
            prompt, base = K.window_prompt(cfg, C, full, win, r)
            q0, tokens = base - off, len(prompt)
            assert q0 >= 0 and (k > 0 or q0 == 0), "window 0 produces result position 0"
            if final:
                new, budget = n - q0, min(max_new, block - tokens)
                assert new >= 0 and out.windows[b][-1][3] == new
                if stopped:
                    assert new < budget and new % 2 == 0
                elif out.finish[b] == "max_new_tokens":
                    assert new == max_new and tokens + new <= block
                else:
                    assert out.finish[b] == "block_size" and tokens + new == block and new < max_new
                n_rows = new + (1 if stopped else 0)
            else:
                new = n_rows = win[3]
                assert n >= q0 + new, "a non-final window produces its exact count"
            ids_k, Lk = result[q0:q0 + new], L[q0:q0 + n_rows]
            ref = R.forward(w, np.concatenate([prompt, ids_k]), torch.float64, positions=list(range(tokens - 1, tokens - 1 + n_rows))).numpy()
            diff = float(np.abs(Lk.astype(np.float64) - ref).max()) if n_rows else 0.0
            worst = max(worst, diff)
            assert diff <= FLOAT_TOL, f"row {b} window {k}: logits differ from the float64 twin by {diff:.3e}"
            allow = K.allow_of(cfg, final)
            for s in range(n_rows):
                want = int(ids_k[s]) if s < new else cfg.STOP_TOKEN
                tok, dist, kept = R.sample(Lk[s], temperature, top_k, u[b, q0 + s], allow[s % 2])
                steps += 1
                if tok != want:
                    assert dist < window(kept), f"row {b} window {k} step {s}: device token {want}, rule gives {tok}, {dist:.3e} from a boundary"
                    waived += 1
    print(f"largest logit difference {worst:.3e}; waived {waived} of {steps} steps")
    assert waived <= 0.02 * steps
    return worst, waived


def run(dec, srcs, voices, u, S=K.S, H=K.H, max_new=K.MAX_NEW, **kw):
    return dec.to_acoustic_long(srcs, window=S, hop=H, max_new_tokens=max_new, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True,
                                voice=voices, **kw)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("P", VC.PROMPTS)
def test_the_grid_follows_the_protocol(family, P):
    """P + N in {S - 1, S, S + 1, S + H + 1, 2 S + 3}: one to four windows, each length alone (the CPU file's chains) and all five in one call."""
    w, dec = decoder(family)
    vp = VC.prompt(P)
    srcs = [K.source(total - P, seed=P) for total in VC.TOTALS]
    for src in srcs:
        u = VC.draws([(P, len(src))], K.MAX_NEW)
        out = run(dec, [src], [vp], u)
        verify(w, dec, K.CFG, [src], [vp], out, u, K.S, K.H, K.MAX_NEW)
        assert len(out.windows[0]) == len(acoustic_windows(P + len(src), K.S, K.H, K.r, K.BLOCK))
    u = VC.draws([(P, len(s)) for s in srcs], K.MAX_NEW)
    out = run(dec, srcs, vp, u)
    verify(w, dec, K.CFG, srcs, [vp] * len(srcs), out, u, K.S, K.H, K.MAX_NEW)


def carry_prompt(cfg, C, X, S, H, r):
    """What the second call of the self-carry identity is prompted with: ids C[H:S] and, as codes, the first call's raw stream X[r H : r S]."""
    ids = X[r * H:r * S].reshape(-1, 2) - cfg.ACOUSTIC_OFFSET - np.array([0, cfg.codebook_size])
    return VoicePrompt(C[H:S], ids.T.copy(), cfg.SEMANTIC_VOCAB_SIZE)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("N", [K.S + 1, K.S + K.H + 1, 2 * K.S + 3])
def test_the_self_carry_identity_is_exact(family, N):
    """An unprompted row on C' gives stream X. Prompted with ids C'[H:S], the codes of X[r H : r S] and the draws U[r S:], the source C'[S:] gives X[r S:]
    id for id and logit for logit: its window 0 is the first call's window 1, token for token, on the same route. The same through the queue at one slot."""
    S, H, r = K.S, K.H, K.r
    w, dec = decoder(family)
    C = K.source(N, seed=9)
    U = K.draws([N], K.MAX_NEW)
    first = dec.to_acoustic_long([C], window=S, hop=H, max_new_tokens=K.MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=U, return_logits=True)
    X = (first.ids[0] + K.CFG.ACOUSTIC_OFFSET).numpy()
    assert len(X) >= r * S
    vp = carry_prompt(K.CFG, C, X, S, H, r)
    u2 = np.ascontiguousarray(U[:, r * S:])
    for kw in (dict(), dict(slots=1)):
        second = run(dec, [C[S:]], vp, u2, **kw)
        assert torch.equal(second.ids[0], first.ids[0][r * S:]) and second.finish == first.finish, kw
        assert torch.equal(second.logits[0], first.logits[0][r * S:]), "logit for logit"
        assert second.windows[0][0][:3] == (0, min(S, N - H), r * (S - H)) and len(second.windows[0]) == len(first.windows[0]) - 1


def test_one_prompt_shared_by_64_sources_through_8_slots():
    """"Equal to each source run alone, id for id under the protocol": every one of the 64 sources passes §17's protocol on the queue's result, that is, each
    id is what ``gpt_ref.sample`` gives on the device's own logits with that source's own draw, and those logits are within the float bar of the twin on that
    source's own prompt, whatever its neighbours are. Four of them are also run alone and held to the same protocol. Bit equality between an 8-slot tick and a
    one-row call is not asserted: their passes take different routes (§20), as in tests/test_gpt_queue_gpu.py's multi-slot cases."""
    w, dec = decoder("peaky")
    vp = VC.prompt(4, seed=3)
    lengths = [1 + (7 * i) % (2 * K.S) for i in range(64)]
    srcs = [K.source(N, seed=20 + i) for i, N in enumerate(lengths)]
    u = VC.draws([(4, N) for N in lengths], K.MAX_NEW)
    out = run(dec, srcs, vp, u, slots=8)
    verify(w, dec, K.CFG, srcs, [vp] * 64, out, u, K.S, K.H, K.MAX_NEW)
    assert sorted({p[0] for p in out.placement}) == list(range(8)) and len({len(x) for x in out.windows}) >= 3
    for i in (0, 21, 42, 63):
        alone = run(dec, [srcs[i]], vp, u[i:i + 1])
        verify(w, dec, K.CFG, [srcs[i]], [vp], alone, u[i:i + 1], K.S, K.H, K.MAX_NEW)
        assert alone.windows[0] == out.windows[i] or alone.windows[0][:-1] == out.windows[i][:-1], "the same schedule alone and in the queue"


@pytest.mark.parametrize("slots", [None, 3])
def test_prompted_and_unprompted_rows_in_one_call(slots):
    w, dec = decoder("uniform")
    a, b = VC.prompt(2, seed=1), VC.prompt(4, seed=2)
    voices = [a, None, b, None, a, b]
    lengths = [2 * K.S + 1, 2 * K.S + 3, K.S - 4, 1, 3, K.S + K.H]
    srcs = [K.source(N, seed=40 + i) for i, N in enumerate(lengths)]
    u = VC.draws([(0 if v is None else len(v), N) for v, N in zip(voices, lengths)], K.MAX_NEW)
    out = run(dec, srcs, voices, u, **({} if slots is None else {"slots": slots}))
    verify(w, dec, K.CFG, srcs, voices, out, u, K.S, K.H, K.MAX_NEW)
    assert [w0[0][2] for w0 in out.windows] == [6, 0, 12, 0, 6, 12], "window 0 carries r P ids, or none"


@pytest.mark.parametrize("slots", [None, 2])
def test_a_call_without_prompts_is_the_existing_entry_point_bit_for_bit(slots):
    """``voice=[None, ...]`` takes the prompt-free entry point; the prompted entry point with every source at -1 must give the same bits, so it is called
    directly here through a table that no source uses."""
    from audiotoken_amd import voice as V
    w, dec = decoder("peaky")
    lengths = [1, K.S, K.S + 1, 2 * K.S + 3]
    srcs = [K.source(N, seed=60 + i) for i, N in enumerate(lengths)]
    u = K.draws(lengths, K.MAX_NEW)
    kw = {} if slots is None else {"slots": slots}
    want = run(dec, srcs, None, u, **kw)
    raw = dec.last_raw_ids.clone()
    assert all(torch.equal(x, y) for x, y in zip(run(dec, srcs, [None] * 4, u, **kw).ids, want.ids))
    unused = VC.prompt(2)
    real = V.voice_table

    def table_nobody_uses(voice, n, *a):
        sem, codes, lens, _ = real(unused, n, *a)
        return sem, codes, lens, [-1] * n

    V.voice_table = table_nobody_uses
    try:
        got = run(dec, srcs, None, u, **kw)
    finally:
        V.voice_table = real
    assert torch.equal(raw, dec.last_raw_ids) and got.finish == want.finish and got.windows == want.windows and got.ticks == want.ticks
    for x, y, lx, ly in zip(got.ids, want.ids, got.logits, want.logits):
        assert torch.equal(x, y) and torch.equal(lx, ly)


@pytest.mark.parametrize("slots", [None, 1])
def test_a_prompt_code_outside_its_code_book_is_clamped_and_reported(slots):
    """``VoicePrompt`` and ``voice_table`` refuse such a code on the host, so the table is built by hand here: one code equal to ``codebook_size``. The kernel
    clamps it to ``codebook_size - 1`` and sets status bit 1, which the Python call turns into ``ValueError``; with the status ignored, the result is bit
    for bit that of the clamped prompt. A prompt id outside the semantic vocabulary sets bit 0 likewise."""
    from audiotoken_amd import voice as V
    w, dec = decoder("uniform")
    cb = K.CFG.codebook_size
    src = K.source(K.S + K.H + 1, seed=70)
    u = VC.draws([(4, len(src))], K.MAX_NEW)
    base = VC.prompt(4, seed=8)
    codes = base.codes.numpy().copy()
    codes[1, 2] = cb - 1
    clamped = VoicePrompt(base.semantic, codes, K.CFG.SEMANTIC_VOCAB_SIZE)
    kw = {} if slots is None else {"slots": slots}
    want = run(dec, [src], clamped, u, **kw)
    real = V.voice_table

    def bad_table(bad_sem, bad_code):
        def table(voice, n, *a):
            sem, c, lens, of_row = real(clamped, n, *a)
            sem, c = sem.copy(), c.copy()
            if bad_code:
                c[0, 1, 2] = cb
            if bad_sem:
                sem[0, 1] = -5
            return sem, c, lens, of_row
        return table

    try:
        V.voice_table = bad_table(False, True)
        with pytest.raises(ValueError, match="code book"):
            run(dec, [src], clamped, u, **kw)
        assert dec.last_status() & 2 and not dec.last_status() & 1, "status bit 1, and only it"
        dec.last_status = lambda: 0   # look past the report, at what was generated
        try:
            got = run(dec, [src], clamped, u, **kw)
        finally:
            del dec.last_status
        assert torch.equal(got.ids[0], want.ids[0]) and torch.equal(got.logits[0], want.logits[0]), "the code was clamped to codebook_size - 1"
        V.voice_table = bad_table(True, False)
        with pytest.raises(ValueError, match="semantic vocabulary"):
            run(dec, [src], clamped, u, **kw)
        assert dec.last_status() & 1 and not dec.last_status() & 2
    finally:
        V.voice_table = real
    again = run(dec, [src], clamped, u, **kw)
    assert torch.equal(again.ids[0], want.ids[0]) and dec.last_status() == 0


def test_product_geometry():
    """S = 250, H = 124, P = 126 = S - H, N = 249 at a block of 1024: P + N = S + H + 1, three windows; window 0 is prompted with 250 + 1 + 378 tokens and
    produces 372 ids, as an unprompted window 1 does."""
    S, H, P, N = 250, 124, 126, 249
    w, dec = decoder("peaky", block=1024, cfg=K.CFG_PRODUCT)
    vp = VC.prompt(P, seed=5, cfg=K.CFG_PRODUCT)
    src = K.source(N, seed=6, cfg=K.CFG_PRODUCT)
    u = VC.draws([(P, N)], 16, S=S, H=H, block=1024)
    out = run(dec, [src], vp, u, S=S, H=H, max_new=16)
    verify(w, dec, K.CFG_PRODUCT, [src], [vp], out, u, S, H, 16)
    assert [x[:3] for x in out.windows[0]] == [(0, 250, 378), (124, 250, 378), (248, 127, 378)]
    assert [x[3] for x in out.windows[0][:2]] == [372, 372] and len(out.ids[0]) == 744 + out.windows[0][2][3]


def test_refusals_raise_before_any_launch():
    w, dec = decoder("uniform")
    good = K.source(2 * K.S + 3)
    u = K.draws([len(good)], K.MAX_NEW)
    before = run(dec, [good], VC.prompt(4), u)
    raw, status = dec.last_raw_ids, dec._status.clone()
    six = VoicePrompt(np.arange(6), np.zeros((2, 9), dtype=np.int64))
    big = VoicePrompt(np.array([0, 256]), np.zeros((2, 3), dtype=np.int64))
    wide = VoicePrompt(np.arange(2), np.full((2, 3), 512))
    for voice, src in [(six, good), (big, good), (wide, good), ([VC.prompt(2)] * 2, good), ("x", good), (VC.prompt(2), np.zeros(65535, dtype=np.int64))]:
        with pytest.raises(ValueError):
            dec.to_acoustic_long([src], window=K.S, hop=K.H, max_new_tokens=K.MAX_NEW, uniforms=u, voice=voice)
        assert dec.last_raw_ids is raw and torch.equal(dec._status, status), "a refused call reaches neither the library nor the device"
    with pytest.raises(ValueError):
        dec.to_acoustic_long([good], window=8, hop=8, max_new_tokens=K.MAX_NEW, uniforms=u, voice=VC.prompt(2))
    again = run(dec, [good], VC.prompt(4), u)
    assert torch.equal(again.ids[0], before.ids[0])
