"""CPU: the fine stage's history rule. tests/golden/fine_hist_a.npz holds what ``transformers``' ``BarkFineModel.generate`` computes with a
``history_prompt`` on the argmax path (tests/golden/make_golden_fine_history.py); the twin (tests/fine_hist_ref.py on tests/fine_ref.py) is held to it at
``make_golden_fine``'s bars: schedule exact, logits within ``parity.FLOAT_TOL``, ids equal or explained by a recorded top-2 margin below 1e-3, teacher-forced
on HF's own buffers. Then the three statements of the schedule (the twin's, the package's, csrc/fine.h's through the stand-alone program) against each
other and against a walk over the frames; what the GPU file's cases would expose; and the argument checks under the host sanitizers."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiotoken_amd import fine_decoder as FD

from tests import fine_cases as K
from tests import fine_hist_cases as HK
from tests import fine_hist_ref as HR
from tests import fine_ref as R
from tests.parity import FLOAT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = np.load(os.path.join(ROOT, "tests", "golden", "fine_hist_a.npz"))
ID_TIE = 1e-3


def golden_case(m, Th, T):
    key = f"{Th}_{T}"
    return {k: GOLDEN[f"{m}_{k}_{key}"] for k in ("coarse", "codes", "sched", "ids", "margin", "pos", "logits")}


@pytest.mark.parametrize("m", ["a", "b"])
def test_schedule_matches_hf_exactly(m):
    Wd = K.MODELS[m]["block"]
    assert GOLDEN[f"{m}_Th"].tolist() == HK.history_lengths(Wd)
    for Th in HK.history_lengths(Wd):
        h = HR.cells(Th, Wd)
        assert GOLDEN[f"{m}_T_{Th}"].tolist() == HK.row_lengths(Wd, h)
        for T in HK.row_lengths(Wd, h):
            want = [tuple(r) for r in golden_case(m, Th, T)["sched"].tolist()]
            assert HR.fine_windows(T, Wd, h) == want, (m, Th, T)
            assert all(fill > start for start, fill in want), "every window of a row with a history has rel > 0"


@pytest.mark.parametrize("m", ["a", "b"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_first_pass_logits_match_hf(m, dtype):
    Wd, w = K.MODELS[m]["block"], K.weights(m, "peaky")
    worst = 0.0
    for Th, T in HK.grid(Wd):
        g = golden_case(m, Th, T)
        work, h = HR.work_array(g["coarse"].astype(np.int64), Wd, GOLDEN[f"{m}_hist_{Th}"].astype(np.int64))
        pos = g["pos"].astype(np.int64)
        assert pos[0] == h, "window 0 predicts from the first cell after the history"
        got = R.forward(w, work[:Wd], 2, dtype, positions=pos).double().numpy()
        worst = max(worst, float(np.abs(got - g["logits"].astype(np.float64)).max()))
    print(f"model {m} {dtype}: twin against HF logits differ by {worst:.2e}")
    assert worst <= FLOAT_TOL


@pytest.mark.parametrize("m", ["a", "b"])
def test_argmax_generation_matches_hf(m):
    """Every window of every golden case: the buffer as HF had it before each pass (rebuilt from HF's recorded ids), the twin's argmax at every predicted
    position against HF's id; then the write-back rule alone must turn HF's ids into HF's output, with the history cells as they were."""
    Wd, w = K.MODELS[m]["block"], K.weights(m, "peaky")
    explained = total = 0
    for Th, T in HK.grid(Wd):
        g = golden_case(m, Th, T)
        hist = GOLDEN[f"{m}_hist_{Th}"].astype(np.int64)
        work, h = HR.work_array(g["coarse"].astype(np.int64), Wd, hist)
        ids, margin = g["ids"].astype(np.int64), g["margin"].astype(np.float32)
        sched = HR.fine_windows(T, Wd, h)
        assert ids.shape == (len(sched), 6, Wd)
        for k, (start, fill) in enumerate(sched):
            rel = fill - start
            assert fill >= h, "no window writes a history cell"
            assert bool((ids[k, :, :rel] == -1).all()) and bool((ids[k, :, rel:] >= 0).all()) and bool((ids[k, :, rel:] < 1024).all())
            for c in range(2, 8):
                got = R.forward(w, work[start:start + Wd], c, torch.float32, positions=list(range(rel, Wd))).numpy().argmax(-1)
                bad = np.nonzero(got != ids[k, c - 2, rel:])[0]
                total += Wd - rel
                for t in bad:
                    assert margin[k, c - 2, rel + t] < ID_TIE, (m, Th, T, k, c, rel + int(t), float(margin[k, c - 2, rel + t]))
                explained += len(bad)
                work[start + rel:start + Wd, c] = ids[k, c - 2, rel:]
        assert np.array_equal(work[:h], hist[:, -h:].T), "the history is read, never written"
        assert np.array_equal(work[h:h + T].T, g["codes"].astype(np.int64)), (m, Th, T)
    print(f"model {m}: {explained} of {total} ids differ from HF's, each with a recorded top-2 margin below {ID_TIE}")


def test_twin_generate_reproduces_hf_where_no_margin_is_small():
    ran = windows = 0
    for m in ("a", "b"):
        Wd, w = K.MODELS[m]["block"], K.weights(m, "peaky")
        for Th, T in HK.grid(Wd):
            g = golden_case(m, Th, T)
            if float(g["margin"].astype(np.float32).min()) <= ID_TIE:
                continue
            codes, _ = HR.generate(w, g["coarse"].astype(np.int64), GOLDEN[f"{m}_hist_{Th}"].astype(np.int64), None)
            assert np.array_equal(codes, g["codes"].astype(np.int64)), (m, Th, T)
            ran += 1
            windows = max(windows, len(g["sched"]))
    print(f"{ran} rows reproduced end to end, the longest of {windows} windows")
    assert ran >= 6 and windows >= 2


# ---- the schedule's three statements ---------------------------------------------------------------------------------------------------------
def sweep(Wd):
    H = Wd // 2
    hs = sorted({0, 1, 2, H // 2, H - 1, H})
    Ts = sorted({1, 2, H - 1, H, H + 1, Wd - H - 1, Wd - 2, Wd - 1, Wd, Wd + 1, Wd + H - 1, Wd + H, Wd + H + 1, 2 * Wd, 2 * Wd + 3, 5 * Wd + 7})
    return [(T, h) for h in hs for T in Ts + [Wd - h - 1, Wd - h, Wd - h + 1]]


@pytest.mark.parametrize("Wd", [128, 256, 1024])
def test_schedule_twins_agree_with_a_walk_over_the_frames(Wd):
    H = Wd // 2
    for T, h in sweep(Wd):
        if T < 1:
            continue
        sched = HR.fine_windows(T, Wd, h)
        assert FD.fine_windows(T, Wd, h) == sched and HR.brute_force_windows(T, Wd, h) == sched, (T, h)
        if h == 0:
            assert sched == R.fine_windows(T, Wd), "h = 0 is the rule without a history"
        L = max(h + T, Wd)
        written = np.zeros(L, dtype=bool)
        for k, (start, fill) in enumerate(sched):
            assert 0 <= start and start + Wd <= L and h <= fill and 0 <= fill - start <= H, (T, h, k)
            assert h == 0 or fill - start > 0, "rel > 0 in every window of a row with a history"
            assert k == 0 or not (~written[h:fill]).any(), "a window predicts from cells whose frames before it are all filled"
            written[fill:start + Wd] = True
        assert written[h:h + T].all() and not written[:h].any(), "every frame of the row is predicted, no history cell is"
    assert [FD.history_cells(Th, Wd) for Th in (1, H - 1, H, H + 5)] == [1, H - 1, H, H]


def run_tool(args=""):
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "fine_hist_asan"] + (["FINE_HIST_ARGS=" + args] if args else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
    return out.stdout


def test_argument_checks_under_the_sanitizers():
    """Every bad argument of the history forms is refused before a launch; Th = 1, Th = H and Th > H are accepted (tools/fine_hist_args.hip)."""
    assert "fine history argument checks: ok" in run_tool()


@pytest.mark.parametrize("Wd", [128, 256, 1024])
def test_the_librarys_schedule_equals_the_twin(Wd):
    """``fine_windows`` / ``fine_window`` / ``fine_history`` of csrc/fine.h, printed by the stand-alone program, against the twin. The program takes
    history FRAMES, so H + 5 frames must come out as H cells."""
    H = Wd // 2
    pairs = [(T, h) for T, h in sweep(Wd) if T >= 1] + [(Wd, H + 5), (1, 4 * Wd)]
    lines = run_tool("sched " + str(Wd) + " " + " ".join(f"{T} {Th}" for T, Th in pairs)).split("\n")
    at = 0
    for T, Th in pairs:
        h = min(H, Th)
        want = HR.fine_windows(T, Wd, h)
        assert lines[at].split() == ["row", str(h), str(max(h + T, Wd)), str(len(want))], (T, Th, lines[at])
        got = [tuple(int(x) for x in ln.split()) for ln in lines[at + 1:at + 1 + len(want)]]
        assert got == want, (T, Th)
        at += 1 + len(want)


# ---- what the GPU file's cases would expose ---------------------------------------------------------------------------------------------------
def test_dropped_or_shifted_history_would_be_exposed():
    c = HK.DROPPED
    w, Wd = K.weights(c["model"], c["family"]), K.MODELS[c["model"]]["block"]
    row, hist = K.coarse_row(c["T"], c["seed"]), HK.history(c["Th"], c["seed"])
    work, h = HR.work_array(row, Wd, hist)
    assert h + c["T"] == Wd, "every key of the window is a real frame"
    frames = list(range(h, Wd))
    whole = R.forward(w, work, 2, torch.float64, positions=frames)
    dropped = R.forward(w, R.work_array(row, Wd), 2, torch.float64, positions=list(range(c["T"])))       # the same frames with no history in front
    shifted_hist = np.concatenate([hist[:, :1], hist[:, :-1]], axis=1)                                   # the history one frame late
    shifted = R.forward(w, HR.work_array(row, Wd, shifted_hist)[0], 2, torch.float64, positions=frames)
    coarse_only = work.copy()
    coarse_only[:h, 2:] = R.VOCAB                                                                        # a history of two channels only
    partial = R.forward(w, coarse_only, 7, torch.float64, positions=frames)
    whole7 = R.forward(w, work, 7, torch.float64, positions=frames)
    for name, moved in (("dropped", (whole - dropped).abs().amax(-1)), ("shifted by one frame", (whole - shifted).abs().amax(-1)),
                        ("without its fine channels", (whole7 - partial).abs().amax(-1))):
        print(f"a history {name} moves the logits by {float(moved.max()):.3e}, at the least moved frame {float(moved.min()):.3e} "
              f"({float(moved.min()) / FLOAT_TOL:.0f} times the bar)")
        assert float(moved.min()) > 8 * FLOAT_TOL, name


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_gpu_seed_keeps_the_twins_own_generation_off_the_boundaries(m, family):
    """The GPU file's draws against the twin's OWN float32 generation on the grid's longest case (Th = H + 5, T = W + H + 1: four windows): at most 2 % of
    the draws may lie inside ``fine_ref.WINDOW``, or the GPU tests would lean on the waiver by construction."""
    Wd = K.MODELS[m]["block"]
    Th, T = Wd // 2 + 5, Wd + Wd // 2 + 1
    h = HR.cells(Th, Wd)
    _, dist = HR.generate(K.weights(m, family), K.coarse_row(T), HK.history(Th), K.TEMPERATURE, HK.draws([(T, h)], Wd)[0])
    inside = int((dist < R.WINDOW).sum())
    print(f"model {m} {family}: {inside} of {dist.size} draws inside the window {R.WINDOW:.2e}; the closest at {dist.min():.2e}")
    assert dist.size == 6 * sum(Wd - (fill - start) for start, fill in HR.fine_windows(T, Wd, h)) and inside <= K.WAIVER_CAP * dist.size


def test_interface_refusals():
    bad = [np.zeros((7, 5), dtype=np.int64), np.zeros((8, 0), dtype=np.int64), np.zeros((8, 5), dtype=np.float32), np.zeros(5, dtype=np.int64)]
    for hst in bad:
        with pytest.raises(ValueError, match="history"):
            FD._as_histories(hst, 2, 128)
    with pytest.raises(ValueError, match="one per row"):
        FD._as_histories([np.zeros((8, 5), dtype=np.int64)], 2, 128)
    shared = np.zeros((8, 70), dtype=np.int64)
    table, of_row, cells = FD._as_histories(shared, 3, 128)
    assert len(table) == 1 and of_row == [0, 0, 0] and cells == [64, 64, 64], "one shared history is one table entry"
    table, of_row, cells = FD._as_histories([shared, None, np.zeros((8, 3), dtype=np.int64)], 3, 128)
    assert len(table) == 2 and of_row == [0, -1, 1] and cells == [64, 0, 3]
    assert FD._as_histories(None, 2, 128) == ([], [-1, -1], [0, 0])
    from audiotoken_amd import AudioToken
    from audiotoken_amd.configs import Tokenizers
    at = AudioToken(Tokenizers.acoustic, device="cuda:0")
    with pytest.raises(ValueError, match="history"):
        at.to_fine(np.zeros((2, 5), dtype=np.int64), history=np.zeros((2, 5), dtype=np.int64))   # refused before any model is built
