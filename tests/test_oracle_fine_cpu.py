"""CPU: the fine stage's twin (tests/fine_ref.py) against an independent implementation: tests/golden/fine_a.npz holds what ``transformers``'
``BarkFineModel`` and its ``generate`` compute for two small seeded models (tests/golden/make_golden_fine.py). The window schedule must match exactly,
logits within ``parity.FLOAT_TOL``, and the argmax ids must be equal or explained by a recorded top-2 margin below 1e-3, the project's bar for ids. The
ids are compared teacher-forced, window by window on HF's own buffers, so a near-tie cannot cascade and a wrong id cannot hide behind one."""
import os

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W

from tests import fine_ref as R
from tests.parity import FLOAT_TOL

GOLDEN = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fine_a.npz"))
MODELS = {"a": dict(block=128, n_layer=2, hidden=768, bias=False), "b": dict(block=256, n_layer=1, hidden=1024, bias=True)}
ID_TIE = 1e-3


@pytest.fixture(scope="module")
def weights():
    return {m: W.synth_fine_weights(k["n_layer"], k["hidden"], k["block"], seed=0, family="peaky", bias=k["bias"]) for m, k in MODELS.items()}


def lengths(Wd):
    H = Wd // 2
    return [1, H, Wd - 1, Wd, Wd + 1, Wd + H, Wd + H + 1, 2 * Wd + 3]


@pytest.mark.parametrize("m", ["a", "b"])
def test_schedule_matches_hf_exactly(m):
    Wd = MODELS[m]["block"]
    assert GOLDEN[f"{m}_T"].tolist() == lengths(Wd)
    for T in lengths(Wd):
        assert R.fine_windows(T, Wd) == [tuple(r) for r in GOLDEN[f"{m}_sched_{T}"].tolist()], (m, T)


@pytest.mark.parametrize("m", ["a", "b"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_logits_match_hf(weights, m, dtype):
    buf, pos = GOLDEN[f"{m}_buf"].astype(np.int64), GOLDEN[f"{m}_pos"].astype(np.int64)
    for c in (2, 5, 7):
        got = R.forward(weights[m], buf, c, dtype, positions=pos).double().numpy()
        diff = float(np.abs(got - GOLDEN[f"{m}_logits_c{c}"].astype(np.float64)).max())
        print(f"model {m} code book {c} {dtype}: twin against HF logits differ by {diff:.2e}")
        assert got.shape == (24, 1024) and diff <= FLOAT_TOL


@pytest.mark.parametrize("m", ["a", "b"])
def test_argmax_generation_matches_hf(weights, m):
    """Every window of every golden length: the buffer as HF had it before each pass (rebuilt from HF's recorded ids), the twin's argmax at every
    predicted position against HF's id; then the write-back rule alone must turn HF's ids into HF's output."""
    Wd = MODELS[m]["block"]
    explained = total = 0
    for T in lengths(Wd):
        work = R.work_array(GOLDEN[f"{m}_coarse_{T}"].astype(np.int64), Wd)
        ids, margin = GOLDEN[f"{m}_ids_{T}"].astype(np.int64), GOLDEN[f"{m}_margin_{T}"]
        sched = R.fine_windows(T, Wd)
        assert ids.shape == (len(sched), 6, Wd)
        for k, (start, fill) in enumerate(sched):
            rel = fill - start
            assert bool((ids[k, :, :rel] == -1).all()) and bool((ids[k, :, rel:] >= 0).all()) and bool((ids[k, :, rel:] < 1024).all())
            for c in range(2, 8):
                logits = R.forward(weights[m], work[start:start + Wd], c, torch.float32, positions=list(range(rel, Wd))).numpy()
                got = logits.argmax(-1)
                bad = np.nonzero(got != ids[k, c - 2, rel:])[0]
                total += Wd - rel
                for t in bad:
                    assert margin[k, c - 2, rel + t] < ID_TIE, (m, T, k, c, rel + int(t), float(margin[k, c - 2, rel + t]))
                explained += len(bad)
                work[start + rel:start + Wd, c] = ids[k, c - 2, rel:]      # HF's ids, padding positions included
        assert np.array_equal(work[:T].T, GOLDEN[f"{m}_codes_{T}"].astype(np.int64)), (m, T)
    print(f"model {m}: {explained} of {total} ids differ from HF's, each with a recorded top-2 margin below {ID_TIE}")


def test_twin_generate_reproduces_hf_where_no_margin_is_small(weights):
    """The twin's own loop end to end, on the lengths whose every recorded margin is above the bar (a near-tie may cascade, so the others are covered by the
    teacher-forced test alone). The golden file must leave a row of more than one window among them."""
    ran = windows = 0
    for m in MODELS:
        Wd = MODELS[m]["block"]
        for T in lengths(Wd):
            if float(GOLDEN[f"{m}_margin_{T}"].min()) <= ID_TIE:
                continue
            codes, _ = R.generate(weights[m], GOLDEN[f"{m}_coarse_{T}"].astype(np.int64), None)
            assert np.array_equal(codes, GOLDEN[f"{m}_codes_{T}"].astype(np.int64)), (m, T)
            ran += 1
            windows = max(windows, len(R.fine_windows(T, Wd)))
    print(f"{ran} rows reproduced end to end, the longest of {windows} windows")
    assert ran >= 3 and windows >= 2
