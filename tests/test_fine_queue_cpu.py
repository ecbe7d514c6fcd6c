"""CPU: the fine stage's window queue without a device: the scheduler's invariants over a sweep of lengths and slots; the library's own
scheduler (csrc/fine.h ``FineQueueSchedule``), dry-run by a stand-alone program under the host sanitizers (tools/fine_queue_args.hip), pass for pass
against the Python twin; the refusal paths through the same program; what the twin alone says about the GPU file's inputs (few draws near a CDF
boundary); and the interface's refusals that need no device."""
import os
import subprocess

import numpy as np
import pytest

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd.fine_decoder import FineGeneration, fine_queue_passes, fine_windows, row_uniforms

from tests import fine_cases as K
from tests import fine_queue_cases as Q
from tests import fine_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def sweep():
    for W in (128, 256, 1024):
        H = W // 2
        sets = [Q.mixed_lengths(W), Q.single_slot_lengths(W), [H] * 130, [1], [40 * W + 7] + [H] * 9, [3 * W, 1, 1, 1, 2 * W + 1, W + 1, 5 * W] * 5]
        for lens in sets:
            for slots in (1, 2, 3, 4, 7, 64):
                yield W, lens, slots


def test_scheduler_invariants():
    n_cases = 0
    for W, lens, slots in sweep():
        passes, placement = fine_queue_passes(lens, W, slots)
        n = [len(fine_windows(T, W)) for T in lens]
        n_cases += 1
        ran = [[] for _ in lens]                 # per row: (k, pass, slot)
        for p, windows in enumerate(passes):
            assert 1 <= len(windows) <= slots, "no pass is empty or over slots"
            assert [j for j, _, _ in windows] == sorted({j for j, _, _ in windows}), "slot order, a slot once per pass: a row never has two windows in one pass"
            for j, b, k in windows:
                ran[b].append((k, p, j))
        first = []
        for b, seq in enumerate(ran):
            assert [k for k, _, _ in seq] == list(range(n[b])), "every window runs once and in order"
            assert [p for _, p, _ in seq] == list(range(seq[0][1], seq[0][1] + n[b])), "a row's windows run in consecutive passes"
            assert len({j for _, _, j in seq}) == 1, "in one slot"
            assert placement[b] == (seq[0][2], seq[0][1], seq[-1][1])
            first.append(seq[0][1])
        assert first == sorted(first), "rows are admitted in the caller's order"
        for p, windows in enumerate(passes):     # rows admitted in one pass take slots in order
            new = [(j, b) for j, b, k in windows if k == 0]
            assert [b for _, b in new] == sorted(b for _, b in new)
        tenures = {}
        for b, (j, lo, hi) in enumerate(placement):
            tenures.setdefault(j, []).append((lo, hi))
        for spans in tenures.values():
            assert all(a[1] < b[0] for a, b in zip(spans, spans[1:])), "a slot never holds two rows"
        # the pass count the rule implies: each row goes to the slot that frees first (the lowest among equals), and a slot is busy for n passes
        free = [0] * slots
        for b in range(len(lens)):
            j = min(range(slots), key=lambda s: (free[s], s))
            assert placement[b][:2] == (j, free[j])
            free[j] += n[b]
        assert len(passes) == max(free)
        assert sum(len(w) for w in passes) == sum(n)
        if slots >= len(lens):
            assert passes == [[(b, b, k) for b in range(len(lens)) if n[b] > k] for k in range(max(n))], "with a slot per row the passes are the lockstep call's"
    assert n_cases == 3 * 6 * 6


def test_scheduler_refusals_and_defaults():
    for lens, slots in (([5], 0), ([5], 65), ([], 4), ([5, 0], 4), ([1] * 4097, 4)):
        with pytest.raises(ValueError):
            fine_queue_passes(lens, 128, slots)
    assert fine_queue_passes([300, 1, 129, 64], 128, 2) == ([[(0, 0, 0), (1, 1, 0)], [(0, 0, 1), (1, 2, 0)], [(0, 0, 2), (1, 2, 1)], [(0, 0, 3), (1, 3, 0)]],
                                                            [(0, 0, 3), (1, 0, 0), (1, 1, 2), (1, 3, 3)])
    assert FineGeneration(codes=[]).passes is None and FineGeneration(codes=[]).placement is None
    u = row_uniforms(3, 5, 2, 128)
    assert u.dtype == np.float32 and u.shape == (2, 6, 128) and bool(((u >= 0) & (u < 1)).all())
    assert np.array_equal(u, np.random.Generator(np.random.Philox(key=[3, 5])).random((2, 6, 128), dtype=np.float32))
    assert np.array_equal(row_uniforms(3, 5, 4, 128)[:2], u), "a row's draws do not depend on how many windows are asked for"
    assert not np.array_equal(row_uniforms(3, 6, 2, 128), u) and not np.array_equal(row_uniforms(4, 5, 2, 128), u)


def run_tool(args=""):
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "fine_queue_asan"] + (["FINE_QUEUE_ARGS=" + args] if args else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
    return out.stdout


def test_argument_checks_under_the_sanitizers():
    assert "fine queue argument checks: ok" in run_tool()


def test_the_librarys_scheduler_equals_the_twin():
    """The same sweep through ``FineQueueSchedule`` (csrc/fine.h), dry-run by the stand-alone program: its passes and placement must equal
    ``fine_queue_passes``'."""
    run_tool()   # builds it once
    exe = os.path.join(ROOT, "audiotoken_amd", "csrc", "build_asan", "fine_queue_args")
    n_cases = 0
    for W, lens, slots in sweep():
        out = subprocess.run([exe, "dry", str(W), str(slots)] + [str(T) for T in lens], capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        got_passes, got_counts = [], []
        for l in lines:
            if l.startswith("pass "):
                windows, counts = l[5:].split(" | ")
                got_passes.append([tuple(int(x) for x in w.split(":")) for w in windows.split()])
                got_counts.append(tuple(int(x) for x in counts.split()))
        got_place = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("row ")]
        passes, placement = fine_queue_passes(lens, W, slots)
        assert got_passes == passes and got_place == placement, (W, slots, lens[:8])
        assert got_counts == [(sum(1 for _, _, k in w if k == 0), sum(1 for b in range(len(lens)) if placement[b][2] == p)) for p, w in enumerate(passes)]
        assert f"passes {len(passes)}" in lines
        n_cases += 1
    assert n_cases == 3 * 6 * 6
    for bad in (["dry", "100", "4", "5"], ["dry", "128", "0", "5"], ["dry", "128", "65", "5"], ["dry", "128", "4", "0"], ["dry", "128", "4", str((1 << 18) + 1)]):
        out = subprocess.run([exe] + bad, capture_output=True, text=True, timeout=120)
        assert out.returncode == 2 and "refused" in out.stdout


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_gpu_seed_keeps_the_twins_own_generation_off_the_boundaries(m, family):
    """The GPU file's rows and per-row draws (tests/fine_queue_cases.py) against the twin's OWN float32 generation: at most 2 % of the draws of the mixed
    case (the one that runs the protocol with draws) may lie inside the near-boundary window that the GPU protocol waives, or the GPU test would lean
    on the waiver by construction."""
    W = K.MODELS[m]["block"]
    w = K.weights(m, family)
    lengths = Q.mixed_lengths(W)
    inside = total = 0
    for i in range(len(lengths)):
        _, dist = R.generate(w, Q.row(i, lengths[i]), K.TEMPERATURE, Q.draws(i, lengths[i], W))
        inside += int((dist < R.WINDOW).sum())
        total += dist.size
    print(f"model {m} {family}: {inside} of {total} draws inside the window {R.WINDOW:.2e}")
    assert total > 0 and inside <= K.WAIVER_CAP * total


def test_interface_refusals():
    for tok in (Tokenizers.acoustic, Tokenizers.semantic_m):
        at = AudioToken(tok, device="cuda:0")
        for bad in (0, 65, -1, 2.5, "4"):
            with pytest.raises(ValueError, match="slots"):
                at.to_fine(np.zeros((2, 10), dtype=np.int64), slots=bad)
        with pytest.raises(ValueError, match=r"\[2, T\]"):
            at.to_fine([np.zeros((2, 10), dtype=np.int64), np.zeros((2, 0), dtype=np.int64)], slots=4)
    lib = _cabi.load()
    assert lib.at_fine_queue_state_bytes(None, 4, 300) == 0 and "not finalized" in _cabi.last_error()
    assert lib.at_fine_generate_queue(None, None, None, 1, 0.5, 0, None, None, None, None, None, 0, 1, 1, None, 0, None, None, None, None) != 0
    assert "not finalized" in _cabi.last_error()
