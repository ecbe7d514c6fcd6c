"""CPU: the long form of semantic-to-acoustic generation without a device: the schedule against a brute-force walk, its refusals, the library's
own window count, what the twin alone says about the GPU file's inputs (few draws near a CDF boundary; a lost or shifted carry moves the logits far past
the float bar), the public interface's refusals, and the stand-alone argument check under the sanitizers."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd.configs import HubertDecoderConfig, Wav2VecBertDecoderConfig
from audiotoken_amd.semantic_decoder import AcousticGeneration, acoustic_windows, default_window

from tests import gpt_ref as R
from tests import long_form_cases as K
from tests.parity import FLOAT_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEOMETRIES = [(8, 4), (8, 8), (250, 124), (254, 126)]


def lengths(S, H):
    return [1, S - 1, S, S + 1, S + H, S + H + 1, 2 * S + 3]


def brute_force(N, S, H, r):
    """The rule walked id by id: a window starts every H source ids until one reaches the source's end; every source id owns r stream positions, a window
    owns those of its source ids that no earlier window produced, and is shown the ones an earlier window produced for the ids it reads."""
    windows, produced, k = [], 0, 0
    while True:
        start = k * H
        ids = [i for i in range(start, start + S) if i < N]
        last = start + S >= N
        seen = [p for i in ids for p in range(r * i, r * i + r) if p < produced]
        new = None if last else len([p for i in ids for p in range(r * i, r * i + r) if p >= produced])
        windows.append((start, len(ids), len(seen), new))
        if seen:
            assert seen == list(range(r * start, r * start + len(seen))), "the carry is one run from the window's first stream position"
        if last:
            return windows
        produced += new
        k += 1


@pytest.mark.parametrize("S,H", GEOMETRIES)
def test_schedule_against_a_brute_force_walk(S, H):
    r = 3
    for N in lengths(S, H):
        plan = acoustic_windows(N, S, H, r, 1024)
        assert plan == brute_force(N, S, H, r), (N, plan)
        n = len(plan)
        assert n == (1 if N <= S else -(-(N - S) // H) + 1) == _cabi.load().at_gpt_long_num_windows(N, S, H)
        end = 0          # stream positions produced so far
        for k, (start, n_src, carry, new) in enumerate(plan):
            assert start == k * H and n_src == min(S, N - k * H)
            assert carry == (0 if k == 0 else r * (S - H))
            base = r * start + carry
            assert base == end, "every stream position is produced exactly once: a window starts where the one before ended"
            assert base % 2 == 0, "parity is the step's parity for the whole pass"
            if k > 0:
                p_start, _, p_carry, p_new = plan[k - 1]
                # the carry lies inside the stream positions of the window before (those it produced and, where H < S / 2 as at (250, 124), the tail of
                # its own carry) and ends where that window ended, at r ((k - 1) H + S)
                assert r * p_start <= r * start and r * start + carry == r * p_start + p_carry + p_new == r * (p_start + S)
                assert carry <= p_carry + p_new
            if k < n - 1:
                assert n_src == S and new == r * S - carry and S + 1 + carry + new <= 1024, "a non-final window is full and fits"
                end = base + new
            else:
                assert new is None and (n == 1 or S - H < n_src <= S)
        assert N - plan[-1][0] == plan[-1][1], "the last window reaches the source's end"


def test_schedule_refusals_and_defaults():
    for S, H, block in [(7, 4, 1024), (8, 3, 1024), (8, 10, 1024), (8, 0, 1024), (0, 0, 1024), (256, 128, 1024), (16, 8, 64)]:
        with pytest.raises(ValueError):
            acoustic_windows(10, S, H, 3, block)
    assert len(acoustic_windows(10, 254, 126, 3, 1024)) == 1      # 254 + 1 + 762 = 1017 fits, 256 + 1 + 768 does not
    for N in (0, 65537):
        with pytest.raises(ValueError):
            acoustic_windows(N, 8, 4, 3, 64)
    assert len(acoustic_windows(65536, 250, 124, 3, 1024)) == -(-(65536 - 250) // 124) + 1
    lib = _cabi.load()
    assert lib.at_gpt_long_num_windows(10, 7, 4) == 0 and "even" in _cabi.last_error()
    assert lib.at_gpt_long_num_windows(10, 8, 10) == 0 and lib.at_gpt_long_num_windows(0, 8, 4) == 0 and lib.at_gpt_long_num_windows(65537, 8, 4) == 0
    assert HubertDecoderConfig().ids_per_source_token == 3 == Wav2VecBertDecoderConfig().ids_per_source_token
    assert default_window(Wav2VecBertDecoderConfig(), 1024) == (250, 124) and default_window(HubertDecoderConfig(), 1024) == (254, 126)
    assert default_window(K.CFG, 64) == (8, 4)
    assert AcousticGeneration(ids=[], codes=[], finish=[]).windows is None


@pytest.fixture(scope="module")
def chains():
    """The twin's own chained generation on the GPU file's single-row inputs (its seed, sources, geometry and budget), both families."""
    out = {}
    for family in K.FAMILIES:
        w = K.weights(family)
        for N in K.LENGTHS:
            src = K.source(N)
            u = K.draws([N], K.MAX_NEW)
            out[(family, N)] = (src, u[0], K.twin_chain(w, K.CFG, src, u[0]))
    return out


def test_the_twins_own_chain_rarely_meets_a_boundary(chains):
    """The GPU protocol may waive an id where the draw lies within 2 (kept 2^-24 + 2^-22) of a CDF boundary, for at most 2 % of a test's steps. On the twin's
    own chain under the GPU file's seed and inputs the share of such draws stays under that cap, so the GPU tests do not lean on the waiver by construction.
    (The product-geometry case is left out here: its 1100 uncached steps over contexts of 1000 ids would take minutes on a CPU.)"""
    for family in K.FAMILIES:
        inside = steps = 0
        closest = float("inf")
        for N in K.LENGTHS:
            _, _, (stream, finish, trace) = chains[(family, N)]
            plan = acoustic_windows(N, K.S, K.H, K.r, K.BLOCK)
            assert finish in ("stop", "max_new_tokens")
            if finish == "max_new_tokens":
                assert len(stream) == plan[-1][0] * K.r + plan[-1][2] + K.MAX_NEW
            assert [p for p, _, _ in trace][:len(stream)] == list(range(len(stream))), "one draw per stream position"
            for _, dist, kept in trace:
                steps += 1
                inside += dist < 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)
                closest = min(closest, dist)
        print(f"{family}: {inside} of {steps} draws inside the window; the closest is {closest:.2e} from a boundary")
        assert inside <= 0.02 * steps


@pytest.mark.parametrize("family", K.FAMILIES)
def test_a_lost_or_shifted_carry_moves_the_logits_past_the_bar(chains, family):
    """What the GPU file compares are a window's logits given its prompt. With the carry dropped from the prompt, or taken one frame (2 ids) early, the
    twin's logits of the same ids move by more than 8 FLOAT_TOL on every later window of the GPU file's inputs: a device that lost or misplaced the carry cannot
    pass the float bar by accident."""
    w = K.weights(family)
    for N in (K.S + 1, K.S + K.H + 1, 2 * K.S + 3):
        src, _, (stream, _, _) = chains[(family, N)]
        plan = acoustic_windows(N, K.S, K.H, K.r, K.BLOCK)
        for k in range(1, len(plan)):
            start, n_src, carry, new = plan[k]
            prompt, base = K.window_prompt(K.CFG, src, stream, plan[k])
            new_ids = stream[base:base + new] if new is not None else stream[base:]
            if len(new_ids) == 0:
                continue
            head = prompt[:n_src + 1]

            def logits(carried):
                seq = np.concatenate([head, carried, new_ids])
                P = len(head) + len(carried)
                return R.forward(w, seq, torch.float64, positions=list(range(P - 1, P - 1 + len(new_ids)))).numpy()

            right = logits(prompt[n_src + 1:])
            dropped = logits(prompt[:0])
            shifted = logits(stream[K.r * start - 2:K.r * start - 2 + carry])
            for what, other in (("dropped", dropped), ("shifted by one frame", shifted)):
                moved = float(np.abs(other - right).max())
                print(f"{family} N={N} window {k}: carry {what} moves the logits by {moved:.3e}")
                assert moved > 8 * FLOAT_TOL, (N, k, what, moved)


def test_interface_refusals():
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_acoustic(np.arange(4), long_form=True)
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_audio(np.arange(4), long_form=True)
    for tok in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        for kw in (dict(window=8), dict(hop=4), dict(window=8, hop=4)):
            with pytest.raises(ValueError, match="long_form"):
                AudioToken(tok, device="cuda:0").to_acoustic(np.arange(4), **kw)
            with pytest.raises(ValueError, match="long_form"):
                AudioToken(tok, device="cuda:0").to_audio(np.arange(4), **kw)


def test_argument_checks_under_the_sanitizers():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "gpt_long_asan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gpt long-form argument checks: ok" in out.stdout
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
