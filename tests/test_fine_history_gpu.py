"""GPU: the fine stage with a history prompt (csrc/fine.hip) against the twin in tests/fine_hist_ref.py, which
tests/test_fine_history_cpu.py pins to ``BarkFineModel.generate`` with a ``history_prompt``.

The protocol is §18's (tests/test_fine_decoder_gpu.py), per row teacher-forced on the device's own ids: (a) for every (window, code book) the buffer is
rebuilt from the history, the row and ``window_ids``; the float64 twin runs on it, and the device's logits at positions >= rel are within
``parity.FLOAT_TOL``; (b) the device's id equals ``fine_ref.sample`` on the DEVICE's logits with the same draw, waived only within ``fine_ref.WINDOW`` of a
CDF boundary for at most 2 % of a test's draws, never on the argmax path; (c) the output is ``[8, T]``, the row's own frames only, equal to what the
write-back rule makes of the ids; nothing is written below ``rel`` (so not into a history cell either) or past a row's length."""
import numpy as np
import pytest
import torch

from audiotoken_amd.fine_decoder import CoarseToFine, row_uniforms

from tests import fine_cases as K
from tests import fine_hist_cases as HK
from tests import fine_hist_ref as HR
from tests import fine_ref as R
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_decoders = {}


def decoder(m, family):
    if (m, family) not in _decoders:
        _decoders[(m, family)] = CoarseToFine(device=DEV, weights=K.weights(m, family))
    return _decoders[(m, family)]


def verify(w, dec, rows, hists, gen, uniforms, temperature, raw=None):
    """``uniforms``: per row float32 [n_b, 6, W] (or None on the argmax path). ``raw``: [B, 8, max_T], the call's whole output buffer."""
    Wd = dec.block_size
    waived = draws = 0
    worst = 0.0
    seen = {c: [] for c in range(2, 8)}
    for b, coarse in enumerate(rows):
        T = coarse.shape[1]
        work, h = HR.work_array(coarse, Wd, hists[b])
        before = work[:h].copy()
        sched = HR.fine_windows(T, Wd, h)
        L, ids = gen.logits[b].numpy(), gen.window_ids[b].numpy()
        assert L.shape == (len(sched), 6, Wd, 1024) and ids.shape == (len(sched), 6, Wd)
        for k, (start, fill) in enumerate(sched):
            rel = fill - start
            assert fill >= h and (h == 0 or rel > 0)
            assert bool((ids[k, :, :rel] == -1).all()) and bool(np.isnan(L[k, :, :rel]).all()), "nothing is written below rel"
            assert bool((ids[k, :, rel:] >= 0).all()) and bool((ids[k, :, rel:] < 1024).all())
            for c in range(2, 8):
                dev_logits = L[k, c - 2, rel:]
                seen[c].append((b, k, rel, work[start:start + Wd].copy(), dev_logits))
                u = None if temperature is None else uniforms[b][k, c - 2, rel:]
                tok, dist = R.sample_many(dev_logits, temperature, u)
                bad = np.nonzero(tok != ids[k, c - 2, rel:])[0]
                for t in bad:
                    assert temperature is not None, f"row {b} window {k} code book {c} position {rel + t}: the argmax has no waiver"
                    assert dist[t] < R.WINDOW, (f"row {b} window {k} code book {c} position {rel + t}: device id {ids[k, c - 2, rel + t]}, rule gives "
                                                f"{tok[t]}, {dist[t]:.3e} from a boundary (window {R.WINDOW:.3e})")
                waived += len(bad)
                draws += Wd - rel
                work[start + rel:start + Wd, c] = ids[k, c - 2, rel:]
        codes = gen.codes[b].numpy()
        assert codes.shape == (8, T) and gen.codes[b].dtype == torch.int64
        assert np.array_equal(work[:h], before), "no history cell is written"
        assert np.array_equal(codes[:2], coarse), "channels 0 and 1 are the input"
        assert np.array_equal(codes, work[h:h + T].T), "the output is the row's own frames, as the write-back rule makes them of the ids"
        if raw is not None:
            assert np.array_equal(raw[b, :, :T].numpy(), codes) and bool((raw[b, :, T:] == -1).all()), "nothing is written past a row's length"
    for c, items in seen.items():
        for i in range(0, len(items), 32):
            chunk = items[i:i + 32]
            ref = R.forward(w, np.stack([it[3] for it in chunk]), c, torch.float64).numpy()
            for (b, k, rel, _, dev_logits), r in zip(chunk, ref):
                diff = float(np.abs(dev_logits.astype(np.float64) - r[rel:]).max())
                worst = max(worst, diff)
                assert diff <= FLOAT_TOL, f"row {b} window {k} code book {c}: logits differ from the float64 twin by {diff:.3e}"
    print(f"largest logit difference {worst:.3e}; waived {waived} of {draws} draws")
    assert waived <= K.WAIVER_CAP * draws
    return worst, waived


def case_rows(Wd, pairs):
    """rows, histories and the (T, h) list of (Th, T) pairs; Th = 0: no history."""
    rows = [K.coarse_row(T, b) for b, (Th, T) in enumerate(pairs)]
    hists = [HK.history(Th, b) if Th else None for b, (Th, T) in enumerate(pairs)]
    return rows, hists, [(T, HR.cells(Th, Wd)) for Th, T in pairs]


def run(m, family, pairs, temperature=K.TEMPERATURE):
    w, dec = K.weights(m, family), decoder(m, family)
    rows, hists, shape = case_rows(dec.block_size, pairs)
    u = HK.draws(shape, dec.block_size)
    gen = dec.generate(rows, temperature=temperature, uniforms=u, return_logits=True, history=hists)
    verify(w, dec, rows, hists, gen, u, temperature, dec.last_raw_codes)
    return rows, hists, u, gen


@pytest.mark.parametrize("temperature", [None, K.TEMPERATURE])
@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
@pytest.mark.parametrize("which", range(4))
def test_the_goldens_grid(m, family, which, temperature):
    """One history length of the golden's grid per case, its five row lengths as five calls of one row."""
    Wd = K.MODELS[m]["block"]
    Th = HK.history_lengths(Wd)[which]
    for T in HK.row_lengths(Wd, HR.cells(Th, Wd)):
        run(m, family, [(Th, T)], temperature)


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_rows_with_and_without_history_equal_each_row_alone(m, family):
    Wd = K.MODELS[m]["block"]
    H = Wd // 2
    pairs = [(H + 5, Wd + H + 1), (0, Wd + 1), (1, Wd), (0, 1), (H - 1, H + 2), (H, 1)]
    assert [len(HR.fine_windows(T, Wd, HR.cells(Th, Wd))) for Th, T in pairs] == [4, 2, 2, 1, 2, 1]
    rows, hists, u, gen = run(m, family, pairs)
    dec = decoder(m, family)
    for b, row in enumerate(rows):
        n = len(HR.fine_windows(row.shape[1], Wd, HR.cells(pairs[b][0], Wd)))
        alone = dec.generate(row, temperature=K.TEMPERATURE, uniforms=u[b:b + 1, :n], history=hists[b])
        assert torch.equal(alone.codes[0], gen.codes[b]), f"row {b} alone, with its own draws, gives other codes than in the batch"


@pytest.mark.parametrize("m", ["a", "b"])
def test_window_queue_equals_the_lockstep_call(m):
    """Seven rows of mixed Th and T through three slots: windows of different rows, different k and different rel side by side in one pass, and slots that
    take a row with a history after one without. Each row equals the lockstep call's row, and the protocol holds on the queue's own logits."""
    Wd, family = K.MODELS[m]["block"], "peaky"
    H = Wd // 2
    w, dec = K.weights(m, family), decoder(m, family)
    pairs = [(H + 5, Wd + H + 1), (0, 3), (1, Wd), (H, 2 * Wd + 3), (0, Wd + 1), (H - 1, 1), (H, H + 1)]
    rows, hists, shape = case_rows(Wd, pairs)
    n = [len(HR.fine_windows(T, Wd, h)) for T, h in shape]
    u = [row_uniforms(K.SEED, b, n[b], Wd) for b in range(len(rows))]
    q = dec.generate_queue(rows, slots=3, temperature=K.TEMPERATURE, uniforms=u, return_logits=True, history=hists)
    assert sum(p[0] for p in q.passes) == sum(n) and max(p[0] for p in q.passes) == 3
    verify(w, dec, rows, hists, q, u, K.TEMPERATURE)
    lock_u = np.zeros((len(rows), max(n), 6, Wd), dtype=np.float32)
    for b in range(len(rows)):
        lock_u[b, :n[b]] = u[b]
    lock = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=lock_u, history=hists)
    for b in range(len(rows)):
        assert torch.equal(q.codes[b], lock.codes[b]), f"row {b}: the queue and the lockstep call differ"
    shared = hists[0]
    one = dec.generate_queue(rows[:3], slots=2, temperature=None, history=shared)
    each = dec.generate_queue(rows[:3], slots=2, temperature=None, history=[shared, shared.copy(), shared])
    assert all(torch.equal(a, b) for a, b in zip(one.codes, each.codes)), "one shared history equals the same history given per row"


@pytest.mark.parametrize("m", ["a", "b"])
def test_history_none_is_todays_call_bit_for_bit(m):
    Wd, dec = K.MODELS[m]["block"], decoder(m, "uniform")
    lengths = [1, Wd + 1, 2 * Wd + 3]
    rows = [K.coarse_row(T, b) for b, T in enumerate(lengths)]
    u = K.draws(lengths, Wd)
    plain = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=u, return_logits=True)
    none = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=u, return_logits=True, history=None)
    per_row = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=u, return_logits=True, history=[None, None, HK.history(5)])
    for b in range(3):
        assert torch.equal(plain.codes[b], none.codes[b])
        assert torch.equal(plain.logits[b].view(torch.int32), none.logits[b].view(torch.int32)), "the same bits, NaN below rel included"
    # the history form of the entry point with rows that name no entry: the same bits again
    for b in range(2):
        assert torch.equal(plain.codes[b], per_row.codes[b])
        assert torch.equal(plain.logits[b].view(torch.int32), per_row.logits[b].view(torch.int32))
    assert not torch.equal(plain.codes[2], per_row.codes[2]), "a history changes what follows it"
    qu = [row_uniforms(3, b, len(R.fine_windows(T, Wd)), Wd) for b, T in enumerate(lengths)]
    q_plain = dec.generate_queue(rows, slots=2, temperature=K.TEMPERATURE, uniforms=qu)
    q_none = dec.generate_queue(rows, slots=2, temperature=K.TEMPERATURE, uniforms=qu, history=[None] * 3)
    assert all(torch.equal(a, b) for a, b in zip(q_plain.codes, q_none.codes))


def test_dropped_history_cannot_pass():
    """tests/fine_hist_cases.DROPPED: the CPU file shows that a history dropped, shifted by one frame or stripped of its fine channels moves these logits by
    more than 8 times the bar; here they meet it."""
    c = HK.DROPPED
    w, dec = K.weights(c["model"], c["family"]), decoder(c["model"], c["family"])
    row, hist = K.coarse_row(c["T"], c["seed"]), HK.history(c["Th"], c["seed"])
    gen = dec.generate(row, temperature=None, return_logits=True, history=hist)
    work, h = HR.work_array(row, dec.block_size, hist)
    ref = R.forward(w, work, 2, torch.float64).numpy()[h:]
    diff = float(np.abs(gen.logits[0][0, 0, h:].numpy().astype(np.float64) - ref).max())
    print(f"dropped-history case: device against the float64 twin {diff:.3e}")
    assert diff <= FLOAT_TOL
    for cb in range(2, 7):      # the buffer as pass 7 saw it: the row's channels 2 to 6 written, its channel 7 still empty, the history whole
        work[h:, cb] = gen.window_ids[0][0, cb - 2, h:].numpy()
    ref7 = R.forward(w, work, 7, torch.float64).numpy()[h:]
    diff7 = float(np.abs(gen.logits[0][0, 5, h:].numpy().astype(np.float64) - ref7).max())
    print(f"code book 7, which reads every channel of the history: {diff7:.3e}")
    assert diff7 <= FLOAT_TOL


def test_state_reuse_after_a_call_with_history():
    """A slot's work array is longer with a history: a call without one right after must not read what the longer call left behind."""
    Wd = K.MODELS["a"]["block"]
    w, dec = K.weights("a", "uniform"), decoder("a", "uniform")
    dec.generate([K.coarse_row(2 * Wd + 3, 1)], temperature=None, history=HK.history(Wd))
    short = K.coarse_row(Wd // 2, 2)
    again = dec.generate(short, temperature=None, history=HK.history(3))
    fresh = CoarseToFine(device=DEV, weights=w).generate(short, temperature=None, history=HK.history(3))
    assert torch.equal(again.codes[0], fresh.codes[0])


def test_a_history_id_outside_its_range_raises():
    dec = decoder("a", "uniform")
    for value in (1024, -1):
        bad = HK.history(70)
        bad[7, 69] = value
        with pytest.raises(ValueError, match="history id lies outside"):
            dec.generate(K.coarse_row(10), history=bad)
    ok = HK.history(70)
    ok[7, 5] = 5000      # frames before the last H are not read
    assert dec.generate(K.coarse_row(10), temperature=None, history=ok).codes[0].shape == (8, 10), "the handle goes on working"


def test_real_size_window_with_history():
    """W = 1024, Th = 600 (h = 512), T = 1025: three windows, each of rel 512 (the last slid back to the array's end), the head on the gathered rows in each."""
    from audiotoken_amd import weights as W
    w = W.synth_fine_weights(1, 768, 1024, seed=0, family="peaky")
    dec = CoarseToFine(device=DEV, weights=w)
    assert HR.fine_windows(1025, 1024, 512) == [(0, 512), (512, 1024), (513, 1025)]
    rows, hists = [K.coarse_row(1025)], [HK.history(600)]
    u = HK.draws([(1025, 512)], 1024)
    gen = dec.generate(rows, temperature=K.TEMPERATURE, uniforms=u, return_logits=True, history=hists)
    verify(w, dec, rows, hists, gen, u, K.TEMPERATURE, dec.last_raw_codes)


def test_to_fine_passes_the_history_on():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.configs import Tokenizers
    fine_w = K.weights("a", "peaky")
    at = AudioToken(Tokenizers.acoustic, device=DEV, fine_weights=fine_w)
    rows, hist = [K.coarse_row(70), K.coarse_row(200, 1)], HK.history(100)
    dec = decoder("a", "peaky")
    for slots in (None, 2):
        got = at.to_fine(rows, temperature=None, history=hist, slots=slots)
        want = dec.generate(rows, temperature=None, history=hist)
        assert all(torch.equal(a, b) for a, b in zip(got.codes, want.codes))
    assert not torch.equal(at.to_fine(rows, temperature=None).codes[0], want.codes[0])
