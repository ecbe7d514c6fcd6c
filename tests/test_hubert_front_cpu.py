"""CPU: the length table of tests/hubert_front_cases.py reaches what it claims, and the float64 twin plus the bar of tests/test_hubert_front_gpu.py have the
power to see the faults the table is aimed at: a conv that drops or misplaces its last used input row, a conv that reads its unused trailing row, GroupNorm
statistics over the wrong windows, a frame-mask length off by one."""
import numpy as np
import pytest
import torch

from oracle import hubert_ref as R
from tests import hubert_front_cases as H

_W = {}
_REF = {}     # N -> (wave [1, N], float64 features, e_ref)


def _weights():
    if not _W:
        _W.update(H.weights(1))
    return _W


def _ref(N):
    """One clip of length N: its float64 features and e_ref = the fp32 oracle's own distance from them. Computed once, never changed."""
    if N not in _REF:
        wave = H.waveform(N, 1)
        f64 = H.conv_features_f64(_weights(), wave)
        e_ref = (R.conv_features(_weights(), wave).double() - f64).abs().max().item()
        _REF[N] = (wave, f64, e_ref)
    return _REF[N]


def _bar(N):
    """The widest bar tests/test_hubert_front_gpu.py applies to this clip."""
    return max(H.C_BAR.values()) * _ref(N)[2]


def test_every_parity_pattern_occurs_once_in_small():
    sigs = [H.signature(n) for n in H.SMALL]
    assert len(H.SMALL) == 64 and len(set(sigs)) == 64
    assert all(H.chain(n)[7] in (1, 2) for n in H.SMALL)
    # what the rest of the suite encodes reaches 6 of them
    suite = (1200, 4000, 10640, 16000, 32000, 40000, 48000, 48123, 52000, 82000, 96077, 480000)
    assert len({H.signature(n) for n in suite}) == 6


def test_seams_have_the_lengths_they_claim():
    for i, ns in H.SEAM_N.items():
        assert [H.chain(n)[i] for n in ns] == [255, 256, 257], i
        assert list(ns) == [H.smallest_n(i, v) for v in (255, 256, 257)], i
    assert [H.chain(n)[1] for n in (20480,) + H.CHUNK_N] == [4095, 4096, 4097]
    for t, n in H.POSCONV_T.items():
        assert H.chain(n)[7] == t and n == H.smallest_n(7, t)
    for t0, r, n in zip(np.repeat(H.CONV0_T0, 2), [0, 3] * len(H.CONV0_T0), H.CONV0_N):
        assert n >= 10 and H.chain(n)[1] == t0 and (n - 10) % 5 == r
    assert all((n - 10) % 5 != 0 for n in H.RESIDUE) and {(n - 10) % 5 for n in H.RESIDUE} == {1, 2, 3, 4}
    for n in H.TIGHT:
        assert (n - 10) % 5 == 0 and all(H.uses_last_row(n, i) for i in range(1, 7)), n
    assert set(H.IDS_LENGTHS) <= set(H.LENGTHS)
    assert all(H.batch_of(n) == (3 if n < 20000 else 2) for n in H.LENGTHS)


def test_chain_matches_the_oracle_and_the_library():
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    for n in H.LENGTHS + (399, 9, 0):
        assert max(H.chain(n)[7], 0) == max(R.num_frames(n), 0) == lib.at_hubert_num_tokens(n), n


def test_float64_twin_is_the_oracle_in_float64():
    """Same ops, other dtype: the twin and the fp32 oracle agree to fp32 rounding at feature scale, and e_ref is of the order the bar was sized for."""
    for n in (400, 719, 1040):
        _, f64, e_ref = _ref(n)
        scale = f64.abs().max().item()
        print(f"N={n}: feature scale {scale:.2f}, e_ref {e_ref:.3e}")
        assert tuple(f64.shape) == (1, H.chain(n)[7], 512) and f64.dtype == torch.float64
        assert 1.0 < scale < 20.0 and 2.0 ** -24 < e_ref < 64 * 2.0 ** -24 * scale


def _row_edit(conv, row, value):
    def edit(i, h):
        if i == conv:
            h = h.clone()
            h[:, :, row] = value
        return h
    return edit


@pytest.mark.parametrize("conv", range(1, 7))
def test_dropping_the_last_used_row_is_far_above_the_bar(conv):
    """Zero the last input row that conv `conv` uses: on the witness lengths the final features move by more than 1000 bars."""
    for n in H.WITNESS[conv]:
        assert n in H.LENGTHS and all(H.uses_last_row(n, j) for j in range(conv + 1, 7)), (conv, n)
        L = H.chain(n)
        row = 2 * (L[conv + 1] - 1) + H.KERNELS[conv] - 1
        wave, f64, _ = _ref(n)
        moved = (H.conv_features_f64(_weights(), wave, _row_edit(conv, row, 0.0)) - f64).abs()
        print(f"conv {conv}, N={n}: row {row} of {L[conv]} zeroed moves the features by {moved.max().item():.3f}, bar {_bar(n):.2e}")
        assert moved.max().item() > 1000 * _bar(n)
        if moved.shape[1] > 1:      # ... and only in the last frame
            assert moved[:, :-1].max().item() == 0.0


def test_a_row_no_later_conv_uses_does_not_reach_the_features():
    """The other half of the witness rule: at a length where conv 2 leaves its last row unused, conv 1's last used row is invisible in the features —
    which is why the test above names its lengths."""
    n = 410
    assert H.uses_last_row(n, 1) and not H.uses_last_row(n, 2)
    L = H.chain(n)
    wave, f64, _ = _ref(n)
    assert torch.equal(H.conv_features_f64(_weights(), wave, _row_edit(1, 2 * (L[2] - 1) + 2, 0.0)), f64)


@pytest.mark.parametrize("conv", range(1, 7))
def test_the_unused_trailing_row_is_harmless(conv):
    """Where conv `conv` has a trailing input row that no window covers, NaN in that row changes nothing: a kernel that reads it (a padding row of the
    operand plane taken for data) cannot hide behind the reference."""
    for n in H.SLACK[conv]:
        assert n in H.LENGTHS and not H.uses_last_row(n, conv), (conv, n)
        L = H.chain(n)
        assert 2 * (L[conv + 1] - 1) + H.KERNELS[conv] - 1 == L[conv] - 2
        wave, f64, _ = _ref(n)
        got = H.conv_features_f64(_weights(), wave, _row_edit(conv, L[conv] - 1, float("nan")))
        assert torch.isfinite(got).all() and torch.equal(got, f64), (conv, n)


@pytest.mark.parametrize("mutant", ["plus_one", "tail"])
def test_groupnorm_over_the_wrong_windows_is_above_the_bar(mutant):
    """GroupNorm statistics over T0 + 1 windows, or with the uncovered tail samples in the sums: more than 100 bars at a RESIDUE length."""
    seen = {}
    for n in H.RESIDUE:
        wave, f64, _ = _ref(n)
        seen[n] = (H.conv_features_f64(_weights(), wave, gn_windows=mutant) - f64).abs().max().item() / _bar(n)
    print(f"GroupNorm mutant {mutant}: features move by {', '.join(f'N={n}: {v:.0f} bars' for n, v in seen.items())}")
    assert all(v > 100 for v in seen.values())


def test_conv0_twin_of_an_all_zero_clip_is_gelu_beta():
    w = _weights()
    w0, g, b = (H._t64(w, "feature_extractor.conv_layers.0." + k) for k in ("conv.weight", "layer_norm.weight", "layer_norm.bias"))
    y = H.conv0_f64(torch.zeros(2, 403), w0, g, b)
    assert torch.equal(y, torch.nn.functional.gelu(b)[None, :, None].expand_as(y))


def test_frame_mask_length_off_by_one_is_caught_exactly():
    """At the boundary sums 399 / 400 (0 / 1 frame) and 719 / 720 (1 / 2 frames) a length computed from sum - 1, from sum + 1, or with a rounded-up
    division differs from the oracle's mask in at least one entry; the oracle's own lengths are the closed form."""
    sums = (399, 400, 719, 720)
    N, T = 1040, 3
    mask = torch.zeros(len(sums), N)
    for r, s in enumerate(sums):
        mask[r, :s] = 1
    want = R.frame_mask(mask, T)
    assert want.sum(-1).tolist() == [0, 1, 1, 2] == [max(H.frame_len(s), 0) for s in sums]
    holes = torch.zeros(1, N)
    holes[0, ::2] = 1                                        # 520 valid samples scattered to the end: HF counts them, it does not look for the last one
    assert R.frame_mask(holes, T).sum().item() == H.frame_len(520) == 1

    def ceil_len(s):
        for k, st in zip(H.KERNELS, H.STRIDES):
            s = -((k - s) // st) + 1
        return s

    for name, f in (("sum - 1", lambda s: H.frame_len(s - 1)), ("sum + 1", lambda s: H.frame_len(s + 1)), ("ceil", ceil_len)):
        got = torch.arange(T)[None, :] < torch.tensor([f(s) for s in sums])[:, None]
        assert not torch.equal(got, want), name
