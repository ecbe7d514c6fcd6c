"""CPU: the GPT stage's voice prompts without a device: the prompted schedule against a brute-force walk over stream positions and against
the library's own arithmetic (csrc/gpt.h through tools/gpt_voice_args.hip, under the host sanitizers), what the twin alone says about the GPU file's
inputs (few draws near a CDF boundary; a dropped or one-frame-shifted prompt moves the logits far past the float bar), ``VoicePrompt`` and its alignment,
the public interface's refusals, and the stand-alone argument check."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd.semantic_decoder import acoustic_windows, check_prompt, stream_extent, window_steps
from audiotoken_amd.voice import VoicePrompt, per_row, voice_table

from tests import gpt_ref as R
from tests import long_form_cases as K
from tests import voice_cases as VC
from tests.parity import FLOAT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "audiotoken_amd", "csrc")
GEOMETRIES = [(8, 4), (8, 2), (16, 8), (250, 124), (254, 126)]
r = 3


def rows_of(S, H):
    """(P, N): the smallest and the largest prompt, and one between where there is one, with P + N at every length at which the window count changes."""
    out = []
    for P in sorted({2, (S - H) // 4 * 2, S - H} - {0}):
        for total in (S - 1, S, S + 1, S + H, S + H + 1, 2 * S + 3, 1500):
            if total - P >= 1:
                out.append((P, total - P))
    return out


def brute_force(P, N, S, H):
    """The rule walked id by id on the concatenated source: every id owns r stream positions, those of the prompt's ids are given; a window starts every H
    ids until one reaches the end, owns the positions of its ids that nobody produced or gave, and is shown the others."""
    M, windows, have, k = P + N, [], r * P, 0
    while True:
        start = k * H
        ids = [i for i in range(start, start + S) if i < M]
        last = start + S >= M
        own = [p for i in ids for p in range(r * i, r * i + r)]
        seen = [p for p in own if p < have]
        new = None if last else len(own) - len(seen)
        windows.append((start, len(ids), len(seen), new))
        assert seen == list(range(r * start, r * start + len(seen))), "the carry is one run from the window's first stream position"
        if last:
            return windows
        have += new
        k += 1


@pytest.mark.parametrize("S,H", GEOMETRIES)
def test_prompted_schedule_against_a_brute_force_walk(S, H):
    lib = _cabi.load()
    for P, N in rows_of(S, H):
        plan = acoustic_windows(N, S, H, r, 1024, P)
        assert plan == brute_force(P, N, S, H), (P, N, plan)
        assert len(plan) == len(acoustic_windows(P + N, S, H, r, 1024)) == lib.at_gpt_long_num_windows_prompted(P, N, S, H)
        assert plan[0][2] == r * P and (len(plan) == 1 or plan[0][3] == r * S - r * P), "window 0 carries the prompt and produces the rest of r S"
        assert plan[1:] == acoustic_windows(P + N, S, H, r, 1024)[1:], "later windows are unchanged"
        end = r * P
        for k, (start, n_src, carry, new) in enumerate(plan):
            assert r * start + carry == end and end % 2 == 0, "every position past the prompt is produced exactly once, at its parity"
            assert n_src + 1 + carry <= S + 1 + r * (S - H), "no prompt exceeds the unprompted bound"
            end += new or 0
        base, cap, longest = stream_extent([plan], S, r, 10, 1024, [P])
        assert base == [r * plan[-1][0] + plan[-1][2] - r * P] and base[0] >= 0 and cap == base[0] + window_steps(plan, 10, 1024)[-1][1]
    assert acoustic_windows(9, S, H, r, 1024, 0) == acoustic_windows(9, S, H, r, 1024), "prompt length 0 is today's arithmetic"


def test_prompt_refusals():
    for P, N, S, H in [(0, 5, 8, 4), (1, 5, 8, 4), (3, 5, 8, 4), (6, 5, 8, 4), (-2, 5, 8, 4), (2, 0, 8, 4), (4, 65533, 8, 4), (2, 5, 8, 8)]:
        with pytest.raises(ValueError):
            check_prompt(P, N, S, H)
        assert _cabi.load().at_gpt_long_num_windows_prompted(P, N, S, H) == 0
    check_prompt(2, 1, 8, 4), check_prompt(4, 65532, 8, 4), check_prompt(126, 249, 250, 124)
    with pytest.raises(ValueError, match="window - hop"):
        acoustic_windows(5, 8, 4, 3, 64, 6)


@pytest.fixture(scope="module")
def exe():
    out = subprocess.run(["make", "-C", CSRC, "build_asan/gpt_voice_args"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return os.path.join(CSRC, "build_asan", "gpt_voice_args")


@pytest.mark.parametrize("S,H,block,max_new", [(8, 4, 64, 10), (8, 2, 64, 1), (16, 8, 128, 10), (250, 124, 1024, 1024), (254, 126, 1024, 16)])
def test_the_librarys_prompted_geometry_equals_the_twin(exe, S, H, block, max_new):
    rows = rows_of(S, H) + [(0, S + 1), (0, 1)]
    out = subprocess.run([exe, "extent"] + [str(x) for x in (S, H, r, block, max_new)] + [f"{P}:{N}" for P, N in rows], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    got_extent = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("extent ")]
    got_windows = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("window ")]
    plans = [acoustic_windows(N, S, H, r, block, P) for P, N in rows]
    windows = []
    for i, plan in enumerate(plans):
        for k, ((start, n_ids, carry, new), (tokens, budget)) in enumerate(zip(plan, window_steps(plan, max_new, block))):
            windows.append((i, k, n_ids, tokens, budget, 1 if new is None else 0, r * start + carry - r * rows[i][0]))
    _, cap, longest = stream_extent(plans, S, r, max_new, block, [P for P, _ in rows])
    assert got_windows == windows
    assert got_extent == [(longest, cap)]
    bad = subprocess.run([exe, "extent", str(S), str(H), str(r), str(block), "10", f"{S - H + 2}:5"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "refused" in bad.stdout


def test_argument_checks_under_the_sanitizers():
    out = subprocess.run(["make", "-C", CSRC, "gpt_voice_asan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gpt voice prompt argument checks: ok" in out.stdout
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr


@pytest.fixture(scope="module")
def chains():
    """The twin's own chained generation on the GPU file's grid (its seed, prompts, sources, geometry and budget), both families."""
    out = {}
    for family in K.FAMILIES:
        w = K.weights(family)
        for P in VC.PROMPTS:
            vp = VC.prompt(P)
            for total in VC.TOTALS:
                src = K.source(total - P, seed=P)
                u = VC.draws([(P, total - P)], K.MAX_NEW)
                out[(family, P, total)] = (vp, src, VC.twin_chain(w, K.CFG, vp, src, u[0]))
    return out


def test_the_twins_own_chain_rarely_meets_a_boundary(chains):
    """§17's waiver: an id may be waived where the draw lies within 2 (kept 2^-24 + 2^-22) of a CDF boundary, for at most 2 % of a test's steps. Under the GPU
    file's seeds the twin's own draws stay under that cap, so the GPU tests do not lean on it."""
    for family in K.FAMILIES:
        inside = steps = 0
        for P in VC.PROMPTS:
            for total in VC.TOTALS:
                _, _, (stream, finish, trace) = chains[(family, P, total)]
                assert finish in ("stop", "max_new_tokens")
                assert [q for q, _, _ in trace][:len(stream)] == list(range(len(stream))), "one draw per result position, from 0"
                for _, dist, kept in trace:
                    steps += 1
                    inside += dist < 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)
        print(f"{family}: {inside} of {steps} draws inside the window")
        assert inside <= 0.02 * steps


@pytest.mark.parametrize("family", K.FAMILIES)
def test_a_dropped_or_shifted_prompt_moves_the_logits_past_the_bar(chains, family):
    """What the GPU file compares are window 0's logits given its prompt. With the voice prompt dropped (its ids and its carry gone), or its codes taken one
    frame late (2 stream ids), the twin's logits of the same new ids move by more than 8 FLOAT_TOL: a device that lost or misplaced it cannot pass."""
    w = K.weights(family)
    for P in VC.PROMPTS:
        for total in VC.TOTALS:
            vp, src, (stream, _, _) = chains[(family, P, total)]
            plan = acoustic_windows(len(src), K.S, K.H, K.r, K.BLOCK, P)
            given = VC.given_stream(K.CFG, vp)
            full = np.concatenate([given, stream])
            prompt0, base = K.window_prompt(K.CFG, VC.concatenated(vp, src), full, plan[0])
            new_ids = full[base:base + plan[0][3]] if plan[0][3] is not None else full[base:]
            if len(new_ids) == 0:
                continue

            def logits(head):
                seq = np.concatenate([head, new_ids]).astype(np.int64)
                return R.forward(w, seq, torch.float64, positions=list(range(len(head) - 1, len(head) - 1 + len(new_ids)))).numpy()

            n_src = plan[0][1]
            right = logits(prompt0)
            dropped = logits(np.concatenate([np.asarray(src[:n_src - P]) + K.CFG.SEMANTIC_OFFSET, [K.CFG.INFER_TOKEN]]))
            late = np.concatenate([given[2:], given[:2]])   # every frame one early in the carry, the first at its end
            shifted = logits(np.concatenate([prompt0[:n_src + 1], late]))
            for what, other in (("dropped", dropped), ("shifted by one frame", shifted)):
                moved = float(np.abs(other - right).max())
                print(f"{family} P={P} P+N={total}: prompt {what} moves the logits by {moved:.3e}")
                assert moved > 8 * FLOAT_TOL, (P, total, what, moved)


def test_voice_prompt_and_its_alignment():
    vp = VoicePrompt(np.arange(4), np.arange(48).reshape(8, 6))
    assert len(vp) == 4 and vp.frames == 6 and vp.semantic.dtype == torch.int64 and vp.codes.shape == (8, 6)
    assert VoicePrompt(np.arange(2), np.zeros((2, 3), dtype=np.int16)).codes.shape == (2, 3)
    for sem, codes in [(np.arange(3), np.zeros((8, 4), int)), (np.arange(4), np.zeros((8, 5), int)), (np.arange(4), np.zeros((3, 6), int)),
                       (np.arange(0), np.zeros((8, 0), int)), (np.array([0, -1]), np.zeros((8, 3), int)), (np.arange(2), np.full((8, 3), 1024)),
                       (np.arange(2), np.full((8, 3), -1)), (np.arange(2.0), np.zeros((8, 3), int)), (np.arange(2), np.zeros((8, 3)))]:
        with pytest.raises(ValueError):
            VoicePrompt(sem, codes)
    with pytest.raises(ValueError, match="vocabulary"):
        VoicePrompt(np.array([0, 256]), np.zeros((8, 3), int), semantic_vocab=256)
    # the latest aligned stretch: brute force over every even start and length
    for n_ids, frames, max_ids in [(10, 15, 4), (10, 14, 4), (11, 15, 126), (300, 449, 126), (300, 500, 126), (7, 100, 6), (100, 7, 6), (2, 3, 126), (5, 6, 3)]:
        a, P = VoicePrompt.aligned_stretch(n_ids, frames, max_ids)
        fits = [(aa, PP) for PP in range(2, max_ids + 1, 2) for aa in range(0, n_ids, 2) if aa + PP <= n_ids and 3 * (aa + PP) // 2 <= frames]
        best_P = max(PP for _, PP in fits)
        assert P == best_P and a == max(aa for aa, PP in fits if PP == best_P), (n_ids, frames, max_ids)
        sem, codes = np.arange(n_ids) % 256, (np.arange(8 * frames).reshape(8, frames) * 7) % 1024
        cut = VoicePrompt.from_tokens(sem, codes[None], max_ids)
        assert np.array_equal(cut.semantic.numpy(), sem[a:a + P]) and np.array_equal(cut.codes.numpy(), codes[:, 3 * a // 2:3 * a // 2 + 3 * P // 2])
    for n_ids, frames, max_ids in [(1, 100, 10), (100, 2, 10), (100, 100, 1)]:
        with pytest.raises(ValueError):
            VoicePrompt.aligned_stretch(n_ids, frames, max_ids)


def test_the_table_shares_entries_and_the_interface_refuses():
    a, b = VC.prompt(2), VC.prompt(4)
    assert voice_table(None, 3, 256, 512, 3) is None and voice_table([None] * 3, 3, 256, 512, 3) is None
    sem, codes, lens, of_row = voice_table([a, None, b, a], 4, 256, 512, 3)
    assert sem.shape == (2, 4) and codes.shape == (2, 2, 6) and lens == [2, 4] and of_row == [0, -1, 1, 0] and sem.dtype == codes.dtype == np.int32
    assert voice_table(a, 64, 256, 512, 3)[3] == [0] * 64, "one prompt shared by every row is one entry"
    for bad in ([a], [a, a, a], "x", [a, 3]):
        with pytest.raises(ValueError):
            per_row(bad, 2)
    with pytest.raises(ValueError):
        voice_table(VoicePrompt(np.array([0, 300]), np.zeros((2, 3), int)), 1, 256, 512, 3)
    for tok in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        with pytest.raises(ValueError, match="long_form"):
            AudioToken(tok, device="cuda:0").to_acoustic(np.arange(4), voice=a)
        with pytest.raises(ValueError, match="long_form"):
            AudioToken(tok, device="cuda:0").to_audio(np.arange(4), voice=a)
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").voice_prompt("clip.wav")
