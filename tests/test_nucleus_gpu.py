"""GPU: the sampler's truncation (csrc/gpt_model.hip: gpt_sample_kernel<true>) against the CPU twin in tests/nucleus_ref.py.

The op (``at_op_nucleus_sample``): the kept count and the threshold equal the twin's on the same logits, waived only where the twin's ``margin`` (the
smallest ``|G(x) / S_K - top_p|`` over K's distinct values) is below ``NUCLEUS_WINDOW``, for at most 2 % of a test's rows and never on a crafted row; the
token equals the twin's draw on the DEVICE's kept set, waived only within §17's draw window of a CDF boundary; the same call twice gives the same bits.
Generation follows tests/test_semantic_decoder_gpu.py's ``verify_generation``, restated with the new twin: (a) the device's logits within
``parity.FLOAT_TOL`` of the float64 twin, teacher-forced on the device's own sequence; (b) the device's id equals the twin's rule applied to the DEVICE's
logits with the same draw, waived only inside one of the two windows, for at most 2 % of a test's steps; (c) the rows end as the finish rules say.
tests/test_nucleus_cpu.py shows on the twin alone that these inputs leave at most half of that cap inside the windows."""
import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.configs import Tokenizers, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import acoustic_windows, nucleus_sample, seeded_uniforms, topk_sample

from tests import gpt_ref as R
from tests import long_form_cases as K
from tests import nucleus_cases as NC
from tests import nucleus_ref as N
from tests.parity import FLOAT_TOL
from tests.test_long_form_gpu import decoder
from tests.test_semantic_decoder_gpu import DEV, SEED, V_SMALL, model, prompts_of, run

pytestmark = pytest.mark.gpu


# ---- the op ---------------------------------------------------------------------------------------------------------------------------------------
def op(z, T, k, p, q, u, allow=None):
    zd, ud = torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(DEV), torch.from_numpy(np.asarray(u, dtype=np.float32)).to(DEV)
    first = [t.cpu().numpy() for t in nucleus_sample(zd, T, k, ud, p, q, allow)]
    again = [t.cpu().numpy() for t in nucleus_sample(zd, T, k, ud, p, q, allow)]
    for a, b in zip(first, again):
        assert np.array_equal(a.view(np.int32), b.view(np.int32)), "the same call twice gives the same bits"
    return first


def check_row(what, z, T, k, p, q, u, allow, tok, kept, thresh, may_waive):
    """One row of an op call against the twin: (set waived, draw waived)."""
    zt, t_thresh, t_kept, margin, _ = N.truncate(z, T, k, p, q, allow)
    set_waived = False
    if (int(kept), np.float32(thresh)) != (t_kept, t_thresh):
        assert may_waive and margin < N.NUCLEUS_WINDOW, (f"{what}: the device keeps {int(kept)} ids down to {thresh!r}, the rule {t_kept} down to {t_thresh!r}; "
                                                          f"{margin:.3e} from the cut (window {N.NUCLEUS_WINDOW:.3e})")
        set_waived = True
    assert int((zt >= np.float32(thresh)).sum()) == int(kept), f"{what}: kept_out is not the size of the set thresh_out gives"
    want, dist, n = N.draw(zt, thresh, u)
    draw_waived = False
    if int(tok) != want:
        assert may_waive and dist < N.draw_window(n), f"{what}: device token {int(tok)}, the rule draws {want}, {dist:.3e} from a boundary (window {N.draw_window(n):.3e})"
        draw_waived = True
    return set_waived, draw_waived


@pytest.mark.parametrize("V", NC.WIDTHS)
def test_op_grid_against_the_twin(V):
    z = NC.grid_rows(V)
    rows = sets = draws = 0
    for T, k, p, q in NC.grid(V):
        tok, kept, thresh = op(z, T, k, p, q, NC.UNIFORMS)
        for b in range(NC.ROWS):
            s, d = check_row(f"V {V} T {T} top_k {k} top_p {p} min_p {q} row {b}", z[b], T, k, p, q, NC.UNIFORMS[b], None, tok[b], kept[b], thresh[b], True)
            rows, sets, draws = rows + 1, sets + s, draws + d
    print(f"V {V}: {rows} rows, waived {sets} kept sets and {draws} draws")
    assert sets <= NC.WAIVER * rows and draws <= NC.WAIVER * rows


def test_op_crafted_rows_are_never_waived():
    for name, z, T, k, p, q, allow, u, want in NC.crafted():
        tok, kept, thresh = op(z[None], T, k, p, q, [u], allow)
        check_row(name, z, T, k, p, q, u, allow, tok[0], kept[0], thresh[0], False)
        assert want is None or int(kept[0]) == want, f"{name}: kept {int(kept[0])}, the case says {want}"


def test_op_with_both_cuts_off_is_the_top_k_sampler():
    for V, k in ((64, 1), (2048, 100), (53376, 100), (53376, 53376)):
        z = NC.grid_rows(V)
        zd, ud = torch.from_numpy(z).to(DEV), torch.from_numpy(NC.UNIFORMS).to(DEV)
        want = topk_sample(zd, 0.8, k, ud)
        for p, q in ((None, None), (1.0, 0.0)):
            tok, kept, thresh = nucleus_sample(zd, 0.8, k, ud, p, q)
            assert torch.equal(tok, want)
            for b in range(NC.ROWS):
                ids, zk = R.kept_values(z[b], 0.8, k)
                assert int(kept[b]) == ids.size and np.float32(thresh[b].item()) == zk.min()


# ---- generation -----------------------------------------------------------------------------------------------------------------------------------
def verify_steps(what, L, ids, stop_token, u_row, allow_of_step, temperature, top_k, top_p, min_p, count):
    """(b) on the logits ``L [n (+ 1 when the row stopped)]`` of one row or window whose ids are ``ids``."""
    for s in range(L.shape[0]):
        want = int(ids[s]) if s < len(ids) else stop_token
        zt, thresh, kept, margin, k_size = N.truncate(L[s], temperature, top_k, top_p, min_p, allow_of_step(s))
        tok, dist, n = N.draw(zt, thresh, u_row[s])
        count["steps"] += 1
        count["smaller"] += kept < k_size
        if tok != want:
            assert margin < N.NUCLEUS_WINDOW or dist < N.draw_window(n), (f"{what} step {s}: device token {want}, the rule gives {tok}; {margin:.3e} from the cut, "
                                                                         f"{dist:.3e} from a boundary (windows {N.NUCLEUS_WINDOW:.3e}, {N.draw_window(n):.3e})")
            count["waived"] += 1


def finish_counts(count):
    print(f"{count['steps']} steps, the nucleus is smaller than the top-k set in {count['smaller']}, waived {count['waived']}; "
          f"largest logit difference {count.get('worst', 0.0):.3e}")
    assert count["waived"] <= NC.WAIVER * count["steps"]
    assert count["smaller"] >= count["steps"] / 2, "the truncation must cut in at least half the steps, or the test shows nothing"


def test_generate_with_truncation_follows_the_rule():
    """at_gpt_generate: four rows of their own prompt lengths, 40 steps."""
    w, dec = model("uniform")
    prompts = prompts_of(NC.GEN_PROMPTS, V_SMALL, seed=24)
    u = seeded_uniforms(SEED + 24, len(prompts), NC.GEN_STEPS)
    ids, finish, logits = dec.generate(prompts, NC.GEN_STEPS, 0.8, 100, -1, uniforms=u, return_logits=True, top_p=NC.TOP_P, min_p=NC.MIN_P)
    count = {"steps": 0, "smaller": 0, "waived": 0, "worst": 0.0}
    raw = dec.last_raw_ids
    for b, prompt in enumerate(prompts):
        P, n, L = len(prompt), len(ids[b]), logits[b].numpy()
        assert finish[b] == "max_new_tokens" and n == NC.GEN_STEPS and L.shape[0] == n
        assert np.array_equal(raw[b, :n].numpy(), ids[b].numpy())
        ref = R.forward(w, np.concatenate([prompt, ids[b].numpy()]), torch.float64, positions=list(range(P - 1, P - 1 + n))).numpy()
        diff = float(np.abs(L.astype(np.float64) - ref).max())
        count["worst"] = max(count["worst"], diff)
        assert diff <= FLOAT_TOL, f"row {b}: logits differ from the float64 twin by {diff:.3e}"
        verify_steps(f"row {b}", L, ids[b].numpy(), -1, u[b], lambda s: None, 0.8, 100, NC.TOP_P, NC.MIN_P, count)
    finish_counts(count)
    # the handle is off again: the unchanged entry point under the unchanged protocol, and the explicit off values give the same bits
    plain, _ = run(w, dec, prompts, NC.GEN_STEPS, seed=SEED + 24)
    off = dec.generate(prompts, NC.GEN_STEPS, 0.8, 100, -1, uniforms=u, top_p=1.0, min_p=0.0)[0]
    assert all(torch.equal(a, b) for a, b in zip(plain, off))
    assert not all(torch.equal(a, b) for a, b in zip(plain, ids)), "the truncation changes what is drawn"


def verify_long(w, dec, srcs, out, u, max_new, top_p, min_p):
    cfg, block = K.CFG, dec.block_size
    count = {"steps": 0, "smaller": 0, "waived": 0, "worst": 0.0}
    for b, src in enumerate(srcs):
        plan = acoustic_windows(len(src), K.S, K.H, K.r, block)
        stream = (out.ids[b] + cfg.ACOUSTIC_OFFSET).numpy()
        n, L, stopped = len(stream), out.logits[b].numpy(), out.finish[b] == "stop"
        assert L.shape[0] == n + (1 if stopped else 0) and cfg.STOP_TOKEN not in stream.tolist()
        assert out.codes[b] is not None and out.codes[b].shape == (2, n // 2), "every id lies in the code book of its parity"
        for k, win in enumerate(plan):
            final = k == len(plan) - 1
            prompt, base = K.window_prompt(cfg, src, stream, win, K.r)
            P = len(prompt)
            if final:
                new, budget = n - base, min(max_new, block - P)
                assert 0 <= new <= budget and (new < budget) == stopped
                rows = new + (1 if stopped else 0)
            else:
                new = rows = win[3]
                assert n >= base + new, "a non-final window produces its exact count"
            ids_k, Lk = stream[base:base + new], L[base:base + rows]
            ref = R.forward(w, np.concatenate([prompt, ids_k]), torch.float64, positions=list(range(P - 1, P - 1 + rows))).numpy()
            diff = float(np.abs(Lk.astype(np.float64) - ref).max())
            count["worst"] = max(count["worst"], diff)
            assert diff <= FLOAT_TOL, f"row {b} window {k}: logits differ from the float64 twin by {diff:.3e}"
            allow = K.allow_of(cfg, final)
            verify_steps(f"row {b} window {k}", Lk, ids_k, cfg.STOP_TOKEN, u[b, base:], lambda s: allow[s % 2], K.TEMPERATURE, K.TOP_K, top_p, min_p, count)
    finish_counts(count)


def test_long_form_with_truncation_follows_the_rule():
    """at_gpt_generate_long: four sources of two windows each."""
    w, dec = decoder("peaky")
    srcs, u = NC.sources(NC.LONG_LENS), NC.long_draws(NC.LONG_LENS)
    kw = dict(window=K.S, hop=K.H, max_new_tokens=NC.LONG_MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True)
    before = dec.to_acoustic_long(srcs, **kw)
    out = dec.to_acoustic_long(srcs, top_p=NC.TOP_P, min_p=NC.MIN_P, **kw)
    assert all(len(x) == 2 for x in out.windows)
    verify_long(w, dec, srcs, out, u, NC.LONG_MAX_NEW, NC.TOP_P, NC.MIN_P)
    for off in (dec.to_acoustic_long(srcs, **kw), dec.to_acoustic_long(srcs, top_p=1.0, min_p=0.0, **kw)):
        assert all(torch.equal(a, b) for a, b in zip(before.ids, off.ids)) and all(torch.equal(a, b) for a, b in zip(before.logits, off.logits)), \
            "with both off the call gives what it gave before the handle was ever set"


def test_queue_with_truncation_follows_the_rule():
    """at_gpt_generate_queue: six sources through two slots, so that four are admitted mid-run."""
    w, dec = decoder("peaky")
    srcs, u = NC.sources(NC.QUEUE_LENS), NC.long_draws(NC.QUEUE_LENS)
    kw = dict(window=K.S, hop=K.H, max_new_tokens=NC.LONG_MAX_NEW, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True, slots=2)
    before = dec.to_acoustic_long(srcs, **kw)
    out = dec.to_acoustic_long(srcs, top_p=NC.TOP_P, min_p=NC.MIN_P, **kw)
    assert sum(1 for p in out.placement if p[1] > 0) >= 4, "sources admitted while others run"
    verify_long(w, dec, srcs, out, u, NC.LONG_MAX_NEW, NC.TOP_P, NC.MIN_P)
    # a source's result does not depend on its neighbours: the lockstep call on the first four gives the same ids
    four = dec.to_acoustic_long(srcs[:4], top_p=NC.TOP_P, min_p=NC.MIN_P, **{**kw, "uniforms": u[:4], "slots": None})
    assert all(torch.equal(a, b) for a, b in zip(four.ids, out.ids[:4]))
    after = dec.to_acoustic_long(srcs, **kw)
    assert all(torch.equal(a, b) for a, b in zip(before.ids, after.ids)) and all(torch.equal(a, b) for a, b in zip(before.logits, after.logits))


def test_to_audio_with_top_p_equals_the_three_stages_by_hand():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.fine_decoder import seeded_uniforms as fine_uniforms
    from tests import fine_cases
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))
    tokens = [(np.arange(20 + 7 * i) * 7 + i) % 1000 for i in range(3)]
    flat = dict(max_new_tokens=24, temperature=20.0)      # the peaky family all but decides every step; flattened, the cut matters
    u1, u2 = seeded_uniforms(31, 3, 24), fine_uniforms(32, 3, 1, 128)
    coarse = sem.to_acoustic(tokens, uniforms=u1, constrain=True, top_p=0.5, **flat)
    plain = sem.to_acoustic(tokens, uniforms=u1, constrain=True, **flat)
    assert not all(torch.equal(a, b) for a, b in zip(coarse.ids, plain.ids)), "top_p reaches the sampler through to_acoustic"
    by_hand = sem.to_fine(coarse.codes, uniforms=u2).codes
    audio, coarse2, fine = sem.to_audio(tokens, uniforms=u1, fine_uniforms=u2, top_p=0.5, **flat)
    assert all(torch.equal(a, b) for a, b in zip(coarse.ids, coarse2.ids)) and all(torch.equal(a, b) for a, b in zip(fine.codes, by_hand))
    dec8 = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8)
    for i in range(3):
        assert torch.equal(audio[i], dec8.decode(by_hand[i].unsqueeze(0))), f"source {i}: to_audio(top_p=) is the three stages composed by hand"
