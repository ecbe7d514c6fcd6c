"""CPU: the host side of teacher-forced scoring (audiotoken_amd/semantic_decoder.py: score_row, long_score_rows, acoustic_stream): what
``score_acoustic`` refuses, the long form's rows against rows written by hand and against the twin's independent builder, and the sequence builder as the
inverse of ``coarse_codes``. No device."""
import os
import subprocess

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd.semantic_decoder import acoustic_stream, coarse_codes, constrained_allow, long_score_rows, prepare_source, score_row

from tests import gpt_score_ref as SR
from tests import long_form_cases as K

CFG = K.CFG            # semantic ids [64, 320), code book 0 [512, 1024), code book 1 [1024, 1536), INFER 1600, STOP 1601; max_source_tokens 8
A, CB = CFG.ACOUSTIC_OFFSET, CFG.codebook_size


def stream_of(n, seed=0):
    """n model ids in the code books of their parities."""
    rng = np.random.default_rng(seed)
    return np.array([A + CB * (s % 2) + int(rng.integers(0, CB)) for s in range(n)], dtype=np.int64)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------------
def test_wrong_tokenizer_is_refused_like_to_acoustic():
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").score_acoustic(np.arange(4), np.zeros((2, 6), dtype=np.int64))


@pytest.mark.parametrize("tok", [Tokenizers.semantic_s, Tokenizers.semantic_m])
def test_over_long_source_is_refused_without_long_form(tok):
    codes = np.zeros((2, 6), dtype=np.int64)
    with pytest.raises(ValueError, match="max_source_tokens"):
        AudioToken(tok, device="cuda:0").score_acoustic(np.arange(300) % 1000, codes)
    with pytest.raises(ValueError, match="long_form"):
        AudioToken(tok, device="cuda:0").score_acoustic(np.arange(4), codes, window=8)
    with pytest.raises(ValueError, match="max_source_tokens"):
        score_row(np.arange(9), stream_of(4), CFG, 64)


def test_a_sequence_longer_than_the_block_is_refused():
    assert score_row(np.arange(8), stream_of(54), CFG, 64)[0].size == 64
    with pytest.raises(ValueError, match="longer than the model's block"):
        score_row(np.arange(8), stream_of(56), CFG, 64)
    assert score_row(np.arange(8), stream_of(54), CFG, 64, include_stop=False)[0].size == 63


def test_long_form_refusals_name_the_condition():
    N = 21                                   # windows at 0, 4, 8, 12, 16 (the last reads 5 ids); the final window's first step is 3 * 16 + 12 = 60
    src = K.source(N)
    rows = lambda n, **kw: long_score_rows(src, stream_of(n), K.S, K.H, CFG, K.BLOCK, **kw)
    with pytest.raises(ValueError, match="shorter than the final window's first step"):
        rows(58)
    with pytest.raises(ValueError, match="odd id count"):
        rows(61)
    # the final window's prompt is 5 + 1 + 12 = 18 tokens, so its budget is 64 - 18 = 46 ids
    with pytest.raises(ValueError, match="longer than the final window's first step plus its budget"):
        rows(60 + 48)
    with pytest.raises(ValueError, match="did not stop"):
        rows(60 + 46)
    assert len(rows(60 + 46, include_stop=False)[0]) == 5
    assert len(rows(60)[0]) == 5 and len(rows(60, include_stop=False)[0]) == 4, "a final window with nothing to score has no row"
    with pytest.raises(ValueError, match="odd id count"):
        score_row(np.arange(4), stream_of(5), CFG, 64)
    with pytest.raises(ValueError):          # the schedule's own conditions
        long_score_rows(src, stream_of(60), 8, 3, CFG, K.BLOCK)
    with pytest.raises(ValueError, match=r"integer \[K >= 2, T\]"):
        acoustic_stream(np.zeros(6, dtype=np.int64), CFG)
    with pytest.raises(ValueError, match="codes must lie"):
        acoustic_stream(np.full((2, 3), CB), CFG)


def test_c_argument_checks_under_the_sanitizers():
    """at_gpt_score, at_gpt_score_state_bytes and at_op_score_rows refuse every bad argument before a launch (tools/gpt_score_args.hip, a stand-alone program
    built with the host sanitizers)."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audiotoken_amd", "csrc")
    out = subprocess.run(["make", "-C", csrc, "gpt_score_asan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "gpt score argument checks: ok" in out.stdout
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr


# ---- the long form's rows ------------------------------------------------------------------------------------------------------------------------
def hand_row(src, lo, hi, stream, c_lo, c_hi, t_hi, stop):
    """source ids [lo, hi) + 64, INFER, stream [c_lo, c_hi) as the carry, stream [c_hi, t_hi) as the targets (+ STOP)."""
    return (list(np.asarray(src[lo:hi]) + 64) + [1600] + list(stream[c_lo:c_hi]) + list(stream[c_hi:t_hi]) + ([1601] if stop else []), hi - lo + 1 + c_hi - c_lo, c_hi)


@pytest.mark.parametrize("N,n_stream,want", [
    # N <= S: one window, the whole stream and STOP are its targets
    (8, 20, lambda s, x: [hand_row(s, 0, 8, x, 0, 0, 20, True)]),
    # N = S + 1: window 0 produces 24 ids; window 1 reads ids [4, 9), carries stream [12, 24) and scores what is left
    (9, 30, lambda s, x: [hand_row(s, 0, 8, x, 0, 0, 24, False), hand_row(s, 4, 9, x, 12, 24, 30, True)]),
    # three windows: window 1 reads [4, 12), carries [12, 24), produces [24, 36); window 2 reads [8, 13), carries [24, 36)
    (13, 40, lambda s, x: [hand_row(s, 0, 8, x, 0, 0, 24, False), hand_row(s, 4, 12, x, 12, 24, 36, False), hand_row(s, 8, 13, x, 24, 36, 40, True)]),
])
def test_long_rows_against_rows_written_by_hand(N, n_stream, want):
    assert (K.S, K.H, K.r) == (8, 4, 3)
    src, stream = K.source(N), stream_of(n_stream, seed=N)
    hand = want(src, stream)
    got, windows = long_score_rows(src, stream, K.S, K.H, CFG, K.BLOCK)
    twin = SR.long_rows(src, stream, K.S, K.H, K.r, CFG.SEMANTIC_OFFSET, CFG.INFER_TOKEN, CFG.STOP_TOKEN)
    assert len(got) == len(twin) == len(hand)
    for (seq, first, base), (t_seq, t_first, t_base), (h_seq, h_first, h_base) in zip(got, twin, hand):
        assert seq.tolist() == h_seq and (first, base) == (h_first, h_base), "the package's rows are the hand-written ones"
        assert t_seq.tolist() == h_seq and (t_first, t_base) == (h_first, h_base), "so are the twin's"
    assert [w[3] for w in windows] == [len(h[0]) - h[1] - (1 if k == len(hand) - 1 else 0) for k, h in enumerate(hand)], "windows carries the counts scored"
    no_stop = long_score_rows(src, stream, K.S, K.H, CFG, K.BLOCK, include_stop=False)[0]
    assert [r[0].tolist() for r in no_stop] == [h[0] for h in hand[:-1]] + [hand[-1][0][:-1]]


@pytest.mark.parametrize("N", K.LENGTHS + [21])
def test_long_rows_equal_the_twin_s_and_tile_the_stream(N):
    src = K.source(N)
    stream = stream_of(K.capacity(N, 6), seed=N)
    got, _ = long_score_rows(src, stream, K.S, K.H, CFG, K.BLOCK)
    twin = SR.long_rows(src, stream, K.S, K.H, K.r, CFG.SEMANTIC_OFFSET, CFG.INFER_TOKEN, CFG.STOP_TOKEN)
    assert [(s.tolist(), f, b) for s, f, b in got] == [(s.tolist(), f, b) for s, f, b in twin]
    targets = np.concatenate([s[f:] for s, f, _ in got])
    assert targets.tolist() == stream.tolist() + [CFG.STOP_TOKEN], "every stream id is a target exactly once, in order, then STOP"
    at = 0
    for s, f, b in got:
        assert b == at
        at += s.size - f


# ---- the sequence builder ------------------------------------------------------------------------------------------------------------------------
def test_sequence_builder_inverts_coarse_codes():
    rng = np.random.default_rng(11)
    for T in (1, 2, 27):
        codes = torch.from_numpy(rng.integers(0, CB, size=(2, T)))
        stream = acoustic_stream(codes, CFG)
        assert stream.shape == (2 * T,) and torch.equal(coarse_codes(stream - A, CB), codes)
        assert np.array_equal(acoustic_stream(torch.cat([codes, codes + 0]), CFG), stream), "[K >= 2, T] uses rows 0 and 1"
        src = rng.integers(0, CFG.SEMANTIC_VOCAB_SIZE, size=5)
        seq, first = score_row(src, stream, CFG, 64)
        prompt = prepare_source(src, CFG)
        assert first == prompt.size and seq[:first].tolist() == prompt.tolist(), "the prompt is to_acoustic's"
        assert seq[first:].tolist() == stream.tolist() + [CFG.STOP_TOKEN] and seq.dtype == np.int32
        assert score_row(src, stream, CFG, 64, include_stop=False)[0].tolist() == seq[:-1].tolist()
    # every target of a built sequence is allowed by the constrained sets, STOP on an even step
    allow = constrained_allow(CFG)
    for s, t in enumerate(seq[first:].tolist()):
        a = allow[s % 2]
        assert a[0] <= t < a[1] or a[2] <= t < a[3], (s, t)
    with pytest.raises(ValueError, match="nothing to score"):
        score_row(src, np.zeros(0, dtype=np.int64), CFG, 64, include_stop=False)
