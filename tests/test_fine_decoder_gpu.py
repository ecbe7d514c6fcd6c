"""GPU: the fine stage (csrc/fine.hip, audiotoken_amd/fine_decoder.py) against the CPU twin in tests/fine_ref.py, which tests/test_oracle_fine_cpu.py pins
to an independent implementation.

The protocol (``verify``), per row teacher-forced on the device's own ids: (a) for every (window, code book) the buffer is rebuilt from ``window_ids``, the
float64 twin runs on it, and the device's logits at positions >= rel are within ``parity.FLOAT_TOL``; (b) the device's id equals ``fine_ref.sample`` on the
DEVICE's logits with the same draw, waived only where the draw lies within ``fine_ref.WINDOW`` of a CDF boundary (the bound derived there from the kernel's
order of additions), for at most 2 % of a test's draws, and never on the argmax path; (c) the output is ``[8, T]`` with channels 0 and 1 the input, equal to
what the write-back rule makes of the ids, entries below ``rel`` and past a row's length untouched. Both (a) and (b) are anchored on the device's ids, so
a near-tie cannot cascade and a wrong id cannot hide."""
import numpy as np
import pytest
import torch

from audiotoken_amd.configs import Tokenizers
from audiotoken_amd.fine_decoder import CoarseToFine

from tests import fine_cases as K
from tests import fine_ref as R
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORD = {"max_logit_diff": 0.0, "waived": 0, "draws": 0}
_decoders = {}


def decoder(m, family):
    if (m, family) not in _decoders:
        _decoders[(m, family)] = CoarseToFine(device=DEV, weights=K.weights(m, family))
    return _decoders[(m, family)]


def verify(w, dec, rows, gen, uniforms, temperature):
    Wd = dec.block_size
    raw = dec.last_raw_codes
    waived = draws = 0
    worst = 0.0
    seen = {c: [] for c in range(2, 8)}      # per code book: (row, window, rel, the buffer the device saw, its logits)
    for b, coarse in enumerate(rows):
        T = coarse.shape[1]
        sched = R.fine_windows(T, Wd)
        L, ids = gen.logits[b].numpy(), gen.window_ids[b].numpy()
        assert L.shape == (len(sched), 6, Wd, 1024) and ids.shape == (len(sched), 6, Wd)
        work = R.work_array(coarse, Wd)
        for k, (start, fill) in enumerate(sched):
            rel = fill - start
            assert bool((ids[k, :, :rel] == -1).all()) and bool(np.isnan(L[k, :, :rel]).all()), "nothing is written below rel"
            assert bool((ids[k, :, rel:] >= 0).all()) and bool((ids[k, :, rel:] < 1024).all())
            for c in range(2, 8):
                dev_logits = L[k, c - 2, rel:]
                seen[c].append((b, k, rel, work[start:start + Wd].copy(), dev_logits))
                # (b) the sampler, exactly, on the device's logits
                u = None if temperature is None else uniforms[b, k, c - 2, rel:]
                tok, dist = R.sample_many(dev_logits, temperature, u)
                bad = np.nonzero(tok != ids[k, c - 2, rel:])[0]
                for t in bad:
                    assert temperature is not None, f"row {b} window {k} code book {c} position {rel + t}: the argmax has no waiver"
                    assert dist[t] < R.WINDOW, (f"row {b} window {k} code book {c} position {rel + t}: device id {ids[k, c - 2, rel + t]}, rule gives {tok[t]}, "
                                                f"{dist[t]:.3e} from a boundary (window {R.WINDOW:.3e})")
                waived += len(bad)
                draws += Wd - rel
                work[start + rel:start + Wd, c] = ids[k, c - 2, rel:]
        # (c) structure
        codes = gen.codes[b].numpy()
        assert codes.shape == (8, T) and gen.codes[b].dtype == torch.int64
        assert np.array_equal(codes[:2], coarse), "channels 0 and 1 are the input"
        assert np.array_equal(codes, work[:T].T), "the output is what the write-back rule makes of the ids"
        assert np.array_equal(raw[b, :, :T].numpy(), codes) and bool((raw[b, :, T:] == -1).all()), "nothing is written past a row's length"
    # (a) the float bar on the buffers the device saw: the float64 twin on up to 32 windows at a time
    for c, items in seen.items():
        for i in range(0, len(items), 32):
            chunk = items[i:i + 32]
            ref = R.forward(w, np.stack([it[3] for it in chunk]), c, torch.float64).numpy()
            for (b, k, rel, _, dev_logits), r in zip(chunk, ref):
                diff = float(np.abs(dev_logits.astype(np.float64) - r[rel:]).max())
                worst = max(worst, diff)
                assert diff <= FLOAT_TOL, f"row {b} window {k} code book {c}: logits differ from the float64 twin by {diff:.3e}"
    print(f"largest logit difference {worst:.3e}; waived {waived} of {draws} draws")
    RECORD["max_logit_diff"] = max(RECORD["max_logit_diff"], worst)
    RECORD["waived"] += waived
    RECORD["draws"] += draws
    assert waived <= K.WAIVER_CAP * draws
    return worst, waived


def run(m, family, lengths, temperature=K.TEMPERATURE, seed=0):
    w, dec = K.weights(m, family), decoder(m, family)
    rows = [K.coarse_row(T, seed + b) for b, T in enumerate(lengths)]
    u = K.draws(lengths, dec.block_size)
    gen = dec.generate(rows, temperature=temperature, uniforms=u, return_logits=True)
    verify(w, dec, rows, gen, u, temperature)
    return rows, u, gen


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
@pytest.mark.parametrize("which", range(8))
def test_single_row_at_every_schedule_edge(m, family, which):
    T = K.lengths(K.MODELS[m]["block"])[which]
    dec = decoder(m, family)
    assert (dec.n_layers, dec.hidden, dec.block_size, dec.has_bias) == tuple(K.MODELS[m][k] for k in ("n_layer", "hidden", "block", "bias"))
    run(m, family, [T])


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_argmax_path_has_no_waiver(m, family):
    Wd = K.MODELS[m]["block"]
    run(m, family, [Wd + Wd // 2 + 1], temperature=None)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_rows_of_different_lengths_equal_each_row_alone(m, family):
    Wd = K.MODELS[m]["block"]
    lengths = [1, Wd, Wd + 1, 2 * Wd + 3]
    assert [len(R.fine_windows(T, Wd)) for T in lengths] == [1, 1, 2, 4]
    rows, u, gen = run(m, family, lengths)
    dec = decoder(m, family)
    for b, row in enumerate(rows):
        n = len(R.fine_windows(lengths[b], Wd))
        alone = dec.generate(row, temperature=K.TEMPERATURE, uniforms=u[b:b + 1, :n])
        assert torch.equal(alone.codes[0], gen.codes[b]), f"row {b} alone, with its own draws, gives other codes than in the batch"


def test_sixty_four_rows_in_one_call():
    Wd = K.MODELS["a"]["block"]
    rows, u, gen = run("a", "peaky", [Wd // 2] * 64)
    assert len({tuple(c[2].tolist()) for c in gen.codes}) == 64, "rows with different inputs and draws"


def test_state_reuse_short_call_after_long():
    Wd = K.MODELS["a"]["block"]
    w = K.weights("a", "uniform")
    dec = decoder("a", "uniform")
    long_rows = [K.coarse_row(2 * Wd + 3, 1), K.coarse_row(Wd + 1, 1)]
    dec.generate(long_rows, temperature=K.TEMPERATURE, uniforms=K.draws([2 * Wd + 3, Wd + 1], Wd))
    short = K.coarse_row(Wd // 2, 2)
    u = K.draws([Wd // 2], Wd)
    again = dec.generate(short, temperature=K.TEMPERATURE, uniforms=u)
    fresh = CoarseToFine(device=DEV, weights=w).generate(short, temperature=K.TEMPERATURE, uniforms=u)
    assert torch.equal(again.codes[0], fresh.codes[0]), "a short call after a long one must not see the long one's state"


def test_real_size_window():
    """W = 1024, one layer, T = 1025: two windows, eight query tiles of the attention kernel, the head restricted to the second window's 513 fill rows."""
    from audiotoken_amd import weights as W
    w = W.synth_fine_weights(1, 768, 1024, seed=0, family="peaky")
    dec = CoarseToFine(device=DEV, weights=w)
    assert R.fine_windows(1025, 1024) == [(0, 0), (1, 512)]
    rows = [K.coarse_row(1025)]
    u = K.draws([1025], 1024)
    gen = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=u, return_logits=True)
    verify(w, dec, rows, gen, u, K.TEMPERATURE)


def test_lost_key_tile_cannot_pass():
    """tests/fine_cases.LOST_KEY: the CPU file shows that losing the last key tile moves these logits by more than 8 times the bar; here they meet it."""
    c = K.LOST_KEY
    w, dec = K.weights(c["model"], c["family"]), decoder(c["model"], c["family"])
    row = K.coarse_row(c["T"], c["seed"])
    gen = dec.generate(row, temperature=None, return_logits=True)
    ref = R.forward(w, R.work_array(row, dec.block_size), 2, torch.float64).numpy()
    diff = float(np.abs(gen.logits[0][0, 0].numpy().astype(np.float64) - ref).max())
    print(f"lost-key case: device against the float64 twin {diff:.3e}")
    assert diff <= FLOAT_TOL


def test_a_code_outside_its_range_raises():
    dec = decoder("a", "uniform")
    bad = K.coarse_row(10)
    bad[1, 3] = 1024
    with pytest.raises(ValueError, match="outside"):
        dec.generate(bad)
    bad[1, 3] = -1
    with pytest.raises(ValueError, match="outside"):
        dec.generate(bad)
    assert dec.generate(K.coarse_row(10), temperature=None).codes[0].shape == (8, 10), "the handle goes on working"


def test_seed_equals_explicit_uniforms():
    from audiotoken_amd.fine_decoder import seeded_uniforms
    dec = decoder("a", "uniform")
    rows = [K.coarse_row(70), K.coarse_row(200)]
    a = dec.generate(rows, temperature=1.0, seed=3)
    b = dec.generate(rows, temperature=1.0, uniforms=seeded_uniforms(3, 2, 3, 128))
    c = dec.generate(rows, temperature=1.0, seed=4)
    greedy = dec.generate(rows, temperature=None)
    assert all(torch.equal(p, q) for p, q in zip(a.codes, b.codes))
    assert not all(torch.equal(p, q) for p, q in zip(a.codes, c.codes)), "another seed gives other draws"
    assert not all(torch.equal(p, q) for p, q in zip(a.codes, greedy.codes)), "temperature 1.0 samples; only None takes the argmax"


def test_to_audio_is_the_three_stages_composed():
    from audiotoken_amd import AudioToken
    from audiotoken_amd import weights as W
    from audiotoken_amd.configs import Wav2VecBertDecoderConfig
    from audiotoken_amd.fine_decoder import seeded_uniforms
    from audiotoken_amd.semantic_decoder import seeded_uniforms as gpt_uniforms
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    fine_w = K.weights("a", "peaky")
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_w)
    tokens = [np.arange(40) % 1000, (np.arange(90) * 7) % 1000]
    u1 = gpt_uniforms(11, 2, 300)
    by_hand_coarse = sem.to_acoustic(tokens, max_new_tokens=300, uniforms=u1, constrain=True)
    frames = [c.shape[1] for c in by_hand_coarse.codes]     # 150 each unless a row drew STOP
    assert min(frames) >= 1
    u2 = seeded_uniforms(12, 2, max(len(R.fine_windows(T, 128)) for T in frames), 128)
    by_hand_fine = sem.to_fine(by_hand_coarse.codes, uniforms=u2)
    audio, coarse, fine = sem.to_audio(tokens, max_new_tokens=300, uniforms=u1, fine_uniforms=u2)
    assert [c.shape for c in coarse.codes] == [(2, T) for T in frames] and [c.shape for c in fine.codes] == [(8, T) for T in frames]
    ac = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8)
    for b in range(2):
        assert torch.equal(fine.codes[b], by_hand_fine.codes[b]) and torch.equal(fine.codes[b][:2], coarse.codes[b])
        want = ac.decode(by_hand_fine.codes[b].unsqueeze(0))
        assert audio[b].shape == (1, 320 * frames[b]) and audio[b].dtype == torch.float32 and bool(torch.isfinite(audio[b]).all())
        assert torch.equal(audio[b], want), "to_audio is bit-equal to the three stages composed by hand"
    # the fine stage is there on every tokenizer
    assert torch.equal(AudioToken(Tokenizers.acoustic, device=DEV, fine_weights=fine_w).to_fine(coarse.codes, uniforms=u2).codes[1], fine.codes[1])
