"""CPU: the sampler's truncation. The twin (tests/nucleus_ref.py) against an independent statement of the nucleus and against masks
recorded from Hugging Face's warpers (tests/golden/nucleus_a.npz); the Python layer's refusals, off values and reset; the C argument checks as a
stand-alone program under the host sanitizers; and, on the twin alone, that the rows of tests/test_nucleus_gpu.py leave at most half of its waiver cap
inside NUCLEUS_WINDOW, so that the cap cannot be what lets a GPU test pass."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import semantic_decoder as SD
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, check_truncation

from tests import long_form_cases as K
from tests import nucleus_cases as NC
from tests import nucleus_ref as N

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "nucleus_a.npz"))


# ---- the twin -------------------------------------------------------------------------------------------------------------------------------------
def stated_nucleus(zt, top_p):
    """The nucleus written out: a descending sort, a cumulative softmax, remove where the mass before exceeds top_p, never the first."""
    order = np.argsort(-zt.astype(np.float64), kind="stable")
    p = np.exp((zt[order] - zt.max()).astype(np.float32).astype(np.float64))   # the rule's p: one fp32 subtraction, then the exponential
    p /= p.sum()
    before = np.cumsum(p) - p
    remove = before > np.float64(np.float32(top_p))
    remove[0] = False
    keep = np.zeros(zt.shape[0], dtype=bool)
    keep[order[~remove]] = True
    return keep


@pytest.mark.parametrize("V", [2, 64, 1001, 4096])
@pytest.mark.parametrize("temperature", [1.0, 0.8, 0.05])
def test_twin_equals_the_stated_nucleus_on_tie_free_rows(V, temperature):
    rng = np.random.default_rng(V)
    for top_p in (1e-6, 0.3, 0.9, 1.0 - 2.0 ** -20):
        for row in range(6):
            z = (rng.standard_normal(V) * 4.0).astype(np.float32)
            while np.unique(N.tempered(z, temperature)).size != V:   # a sort breaks a tie arbitrarily: the statement below holds on tie-free rows
                z = (rng.standard_normal(V) * 4.0).astype(np.float32)
            zt, thresh, kept, margin, k_size = N.truncate(z, temperature, V, top_p)
            assert margin > 1e-12, "the test's own input: the comparison is decided by float64 rounding"
            keep = stated_nucleus(zt, top_p)
            assert np.array_equal(zt >= thresh, keep) and kept == int(keep.sum()) and k_size == V
            assert bool(keep[np.argmax(zt)]), "the maximum always stays"


def test_twin_rules_on_small_rows():
    z = np.log(np.array([0.5, 0.2, 0.2, 0.05, 0.05], dtype=np.float64)).astype(np.float32)
    kept = lambda **kw: N.truncate(z, 1.0, 5, **kw)[2]
    assert kept(top_p=0.4) == 1 and kept(top_p=0.6) == 3 and kept(top_p=0.89) == 3 and kept(top_p=0.91) == 5, "equal values stay or go together"
    assert kept(top_p=None) == 5 and kept(top_p=1.0) == 5 and kept(min_p=None) == 5 and kept(min_p=0.0) == 5, "the off values"
    assert kept(min_p=0.3) == 3 and kept(min_p=0.5) == 1 and kept(min_p=0.05) == 5
    assert kept(top_p=0.91, min_p=0.3) == 3 and kept(top_p=0.4, min_p=0.05) == 1, "both are evaluated on K and intersected"
    # after the top-k, on K's own mass: of K = {0.5, 0.2, 0.2} the mass above the 0.2s is 0.5 / 0.9 = 0.556
    assert N.truncate(z, 1.0, 2, top_p=0.55)[2] == 1 and N.truncate(z, 1.0, 2, top_p=0.56)[2] == 3
    assert N.truncate(z, 1.0, 2, top_p=0.55)[4] == 3, "ties at the top-k threshold are in K"
    tok, n, thresh, margin = N.sample(z, 1.0, 5, 0.95, top_p=0.6)
    assert (tok, n) == (2, 3) and thresh == z[1] and abs(margin - 0.1) < 1e-6
    # min_p is one fp32 subtraction against float32(log(min_p))
    lmin = N.log_min_p(0.05)
    t = np.array([0.0, lmin, np.nextafter(lmin, np.float32(-np.inf))], dtype=np.float32)
    assert N.truncate(t, 1.0, 3, min_p=0.05)[2] == 2


def test_twin_equals_the_recorded_huggingface_masks():
    rows = close = 0
    for i, (T, k, p, q) in enumerate(GOLD["cases"]):
        for z, mask in zip(GOLD[f"logits_{i}"], GOLD[f"mask_{i}"]):
            zt, thresh, kept, margin, _ = N.truncate(z, T, int(k), p if p < 1.0 else None, q if q > 0.0 else None)
            rows += 1
            d = (zt[zt >= np.partition(zt, 512 - int(k))[512 - int(k)]] - zt.max()).astype(np.float64)
            near_min_p = q > 0.0 and float(np.abs(d - np.log(q)).min()) < 4e-5
            if margin < 4e-5 or near_min_p:      # the warpers work in fp32: a cumulative sum of 512 terms (512 2^-24 = 3e-5) and a product decide
                close += 1
                continue
            assert np.array_equal(zt >= thresh, mask), f"case {i}: the twin keeps {kept}, the warpers {int(mask.sum())}"
    assert rows == 54 and close <= 3, f"{close} of {rows} recorded rows are too close to call"


# ---- the GPU tests' inputs do not lean on the waiver -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V", NC.WIDTHS)
def test_grid_rows_leave_half_the_waiver_cap(V):
    z = NC.grid_rows(V)
    rows = inside = cut = 0
    for T, k, p, q in NC.grid(V):
        for b in range(NC.ROWS):
            _, _, kept, margin, k_size = N.truncate(z[b], T, k, p, q)
            rows += 1
            inside += margin < N.NUCLEUS_WINDOW
            cut += kept < k_size
    print(f"V {V}: {inside} of {rows} rows inside the window; the truncation cuts in {cut}")
    assert inside <= 0.5 * NC.WAIVER * rows
    assert V == 1 or cut >= rows // 4, "the grid exercises the cuts"


def test_crafted_rows_are_outside_the_window_and_say_what_they_claim():
    for name, z, T, k, p, q, allow, u, want in NC.crafted():
        zt, thresh, kept, margin, k_size = N.truncate(z, T, k, p, q, allow)
        assert margin >= 10 * N.NUCLEUS_WINDOW, f"{name}: {margin:.3e} from the cut"
        assert want is None or kept == want, f"{name}: the twin keeps {kept}, the case says {want}"
        _, dist, n = N.draw(zt, thresh, u)
        assert dist > N.draw_window(n), f"{name}: the draw is {dist:.3e} from a boundary"
        v_k = np.partition(zt, len(zt) - min(k, len(zt)))[len(zt) - min(k, len(zt))]
        if name == "top_k binds":
            assert thresh == v_k and kept == k_size
        if name in ("top_p binds", "min_p binds"):
            assert thresh > v_k and kept < k_size
        if name.startswith("the path switch"):
            assert k_size == k, "no ties: K has exactly top_k values, on either side of the list's size"
        if name == "ties overflow the list":
            assert k < NC.LIST < k_size
        if name.startswith("two plateaus"):
            assert (k_size <= NC.LIST) == ("V 512" in name)


def test_generation_inputs_cut_and_stay_outside_the_window():
    """The long-form inputs of the GPU tests on the twin alone (an uncached fp32 forward per step): the nucleus is smaller than the top-k set in at least
    half the steps, and at most half the waiver cap lies inside either window."""
    w = K.weights("peaky")
    srcs, u = NC.sources(NC.LONG_LENS), NC.long_draws(NC.LONG_LENS)
    from tests import gpt_ref as R
    steps = inside = smaller = 0
    for b, src in enumerate(srcs[:2]):
        plan = SD.acoustic_windows(len(src), K.S, K.H, K.r, K.BLOCK)
        stream = []
        for k, win in enumerate(plan):
            final = k == len(plan) - 1
            prompt, base = K.window_prompt(K.CFG, src, stream, win, K.r)
            allow = K.allow_of(K.CFG, final)
            seq = prompt
            for s in range(min(NC.LONG_MAX_NEW, K.BLOCK - len(prompt)) if final else win[3]):
                logits = R.forward(w, seq, torch.float32, positions=[len(seq) - 1])[0].numpy()
                zt, thresh, kept, margin, k_size = N.truncate(logits, K.TEMPERATURE, K.TOP_K, NC.TOP_P, NC.MIN_P, allow[s % 2])
                tok, dist, n = N.draw(zt, thresh, u[b, base + s])
                steps += 1
                smaller += kept < k_size
                inside += margin < N.NUCLEUS_WINDOW or dist < N.draw_window(n)
                if final and tok == K.CFG.STOP_TOKEN:
                    break
                stream.append(tok)
                seq = np.append(seq, tok)
    print(f"{steps} steps, the nucleus is smaller in {smaller}, {inside} inside a window")
    assert smaller >= steps / 2 and inside <= 0.5 * NC.WAIVER * steps


# ---- the Python layer -----------------------------------------------------------------------------------------------------------------------------
def test_check_truncation():
    assert check_truncation() == (1.0, 0.0) and check_truncation(None, None) == (1.0, 0.0) and check_truncation(1.0, 0.0) == (1.0, 0.0)
    assert check_truncation(0.9, 0.05) == (0.9, 0.05) and check_truncation(1, 0) == (1.0, 0.0)
    for bad in (0.0, -0.1, 1.0001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"top_p must lie in \(0, 1\]"):
            check_truncation(bad, None)
    for bad in (1.0, -0.1, 2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"min_p must lie in \[0, 1\)"):
            check_truncation(None, bad)


class _Lib:
    """Stands in for the library under a decoder that has no device: records what reaches at_gpt_set_truncation."""

    def __init__(self):
        self.calls = []

    def at_gpt_set_truncation(self, handle, top_p, min_p):
        self.calls.append((top_p, min_p))
        return 0


def _decoder(run):
    dec = object.__new__(SemanticToAcoustic)
    dec.lib, dec.handle, dec.config, dec.block_size, dec.vocab = _Lib(), None, K.CFG, K.BLOCK, K.V
    dec._run = run
    return dec


def _ran(*a, **k):
    return [torch.zeros(2, dtype=torch.int64) + K.CFG.ACOUSTIC_OFFSET], [2], [2], None


def _raises(*a, **k):
    raise RuntimeError("the call failed")


def test_python_layer_sets_the_handle_and_resets_it():
    prompt, src = [np.arange(4, dtype=np.int32)], [K.source(5)]
    for top_p, min_p, want in ((None, None, (1.0, 0.0)), (1.0, 0.0, (1.0, 0.0)), (0.9, None, (0.9, 0.0)), (None, 0.05, (1.0, 0.05)), (0.3, 0.05, (0.3, 0.05))):
        for entry in ("generate", "to_acoustic", "to_acoustic_long", "queue"):
            dec = _decoder(_ran)
            if entry == "generate":
                dec.generate(prompt, 4, top_p=top_p, min_p=min_p)
            elif entry == "to_acoustic":
                dec.to_acoustic(src, max_new_tokens=4, top_p=top_p, min_p=min_p)
            else:
                dec.to_acoustic_long(src, max_new_tokens=4, top_p=top_p, min_p=min_p, slots=2 if entry == "queue" else None)
            assert dec.lib.calls == [want, (1.0, 0.0)], (entry, top_p, min_p, dec.lib.calls)
    # the reset after an exception
    for entry in ("generate", "to_acoustic_long"):
        dec = _decoder(_raises)
        with pytest.raises(RuntimeError, match="the call failed"):
            dec.generate(prompt, 4, top_p=0.9, min_p=0.05) if entry == "generate" else dec.to_acoustic_long(src, max_new_tokens=4, top_p=0.9, min_p=0.05)
        assert dec.lib.calls == [(0.9, 0.05), (1.0, 0.0)]
    # a refusal reaches neither the handle nor the call
    for kw in (dict(top_p=0.0), dict(top_p=1.5), dict(top_p=float("nan")), dict(min_p=1.0), dict(min_p=-0.5), dict(min_p=float("nan"))):
        dec = _decoder(_raises)
        with pytest.raises(ValueError, match="must lie in"):
            dec.generate(prompt, 4, **kw)
        with pytest.raises(ValueError, match="must lie in"):
            dec.to_acoustic(src, max_new_tokens=4, **kw)
        with pytest.raises(ValueError, match="must lie in"):
            dec.to_acoustic_long(src, max_new_tokens=4, **kw)
        assert dec.lib.calls == []


def test_interface_refusals():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.configs import Tokenizers
    for tok in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        with pytest.raises(ValueError, match="top_p must lie"):
            AudioToken(tok, device="cuda:0").to_audio_batch_files(4, "out", token_files=["a.npy"], top_p=0.0)
        with pytest.raises(ValueError, match="min_p must lie"):
            AudioToken(tok, device="cuda:0").to_audio_batch_files(4, "out", token_files=["a.npy"], min_p=1.0)
    lib = _cabi.load()
    assert lib.at_gpt_set_truncation(None, 0.9, 0.0) != 0 and "null handle" in _cabi.last_error()


def test_c_argument_checks_under_the_sanitizers():
    """at_gpt_set_truncation and at_op_nucleus_sample refuse every bad argument before a launch, and a refused call leaves the handle as it was
    (tools/gpt_nucleus_args.hip, a stand-alone program built with the host sanitizers)."""
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "gpt_nucleus_asan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gpt nucleus argument checks: ok" in out.stdout
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
