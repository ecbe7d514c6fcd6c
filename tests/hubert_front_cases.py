"""Length classes of the semantic_s (HuBERT) front end, the table of clip lengths that reaches every one of them, and the float64 twin the tests hold the
HIP front end to.

The conv chain is L[0] = N, L[i+1] = (L[i] - k[i]) // s[i] + 1 with k = (10, 3, 3, 3, 3, 2, 2), s = (5, 2, 2, 2, 2, 2, 2): L[1] = T0 frames out of conv 0,
L[7] = T. Convs 1..6 (stride 2) run as windowed split GEMMs over a PHASE-MAJOR operand (audiotoken_amd/csrc/hubert.hip, make_plan / conv_chain_split): input
row t of conv i lives in plane t % 2 at index t // 2, so plane 1 is one row shorter when L[i] is odd, a k = 3 conv leaves its last input row unused when
L[i] is even, and a k = 2 conv when L[i] is odd. `signature(N)` = the parities of L[1..6]: the 64 patterns are the length classes.

Plain helper for tests/test_hubert_front_cpu.py and tests/test_hubert_front_gpu.py — not a conftest, no fixtures.
"""
import numpy as np
import torch
import torch.nn.functional as F

from audiotoken_amd import weights as W

KERNELS = (10, 3, 3, 3, 3, 2, 2)
STRIDES = (5, 2, 2, 2, 2, 2, 2)
ARITHS = {"f32": 0, "bf16x3": 1, "f16x2": 2}           # option "arith" of at_hubert_set_option
# the bar of the feature check is C_BAR[arith] * e_ref, e_ref = the torch-CPU fp32 oracle's own max |oracle - float64| on the case:
#   the split schemes: 16 — two fp16 pieces carry 22 significand bits, 4 x the unit roundoff of fp32; bf16x3 (24 bits) is held to the same bar
#   (measured 1.93 .. 4.36 and 2.73 .. 4.90, profiles/hubert_front.txt).
#   f32: 8. It started at 4, twice the 1.78 the fp32 attention kernel needed against the same kind of yardstick (profiles/gemm_f32_routes.txt, item 5),
#   and measured 2.26 .. 5.67, above 4 at 47 of 98 lengths of every class alike. Localised with at_op_gemm (profiles/hubert_front.txt, item 3): each
#   fp32 conv GEMM alone is 3.8 .. 10 x the CPU convolution's error at K = 1536 — the fp32 MFMA (16x16x4) adds its products into ONE accumulator in k
#   order (384 steps at the size of the partial sum), the CPU library's blocked kernel keeps many short partial sums — and is the chain
#   tests/test_gemm_f32_routes_gpu.py pins bit for bit on every route. The arithmetic is as designed; 8 is 1.4 x the measured maximum.
C_BAR = {"f32": 8.0, "bf16x3": 16.0, "f16x2": 16.0}
# conv 0 alone (the fp32-output form), per kind of waveform: 4 as above; 8 where the arithmetic as designed measured above 4 (profiles/hubert_front.txt,
# item 4) — the all-zero clip leaves GELU(beta) alone, whose erfc approximant (Abramowitz-Stegun 7.1.26 in fp32) is 4.52 x torch's erf at |beta| <= 0.1;
# at DC offset 10 and T0 = 1 the variance is exactly 0, so the output is beta + (y - mean) * 316 * gamma with y - mean = 0 in exact arithmetic: the kernel's y
# is its fp32 FMA chain (size 30) and its mean the float64 moment, torch's mean is its own y — the chain's rounding times 316 against one rounding: 6.09
# (at most 1.16 at T0 >= 15).
C_CONV0 = {"normalised": 4.0, "dc10": 8.0, "zero": 8.0, "silent_tail": 4.0, "amp1e-4": 4.0, "amp1e3": 4.0}
WEIGHT_SEED = 41


def chain(N: int):
    """[L[0], ..., L[7]]: the length in front of each conv; L[7] = T frames (0 from the first conv whose input is shorter than its kernel)."""
    L = [int(N)]
    for k, s in zip(KERNELS, STRIDES):
        L.append((L[-1] - k) // s + 1 if L[-1] >= k else 0)
    return L


def signature(N: int):
    """(L[1] % 2, ..., L[6] % 2): the parities the phase-major layout of convs 1..6 branches on."""
    return tuple(x % 2 for x in chain(N)[1:7])


def uses_last_row(N: int, i: int) -> bool:
    """Conv i (1..6) consumes the last row of its input: the last window ends at row 2 (L[i+1] - 1) + k - 1 = L[i] - 1."""
    L = chain(N)
    return 2 * (L[i + 1] - 1) + KERNELS[i] - 1 == L[i] - 1


def smallest_n(i: int, want: int) -> int:
    """The smallest N with L[i] == want."""
    n = want
    for k, s in reversed(list(zip(KERNELS[:i], STRIDES[:i]))):
        n = (n - 1) * s + k
    return n


# One length per parity pattern of L[1..6]: L[1] = 79 .. 142, T = 1 or 2.
SMALL = tuple(range(400, 720, 5))
# N = 400 + 320 j: every conv consumes its last input row (T = 1, 2, 3).
TIGHT = (400, 720, 1040)
# trailing samples that no conv-0 window covers, (N - 10) % 5 = 1, 2, 3, 4 and 4: the GroupNorm moments must ignore them.
RESIDUE = (401, 402, 403, 404, 719)
# {conv i: the smallest N with L[i] = 255, 256, 257}: L[i] = 256 is the split GEMM's M tile and the Mp pad of conv i - 1 (i = 7: the last conv's fp32 output)
SEAM_N = {1: (1280, 1285, 1290), 2: (2560, 2570, 2580), 3: (5120, 5140, 5160), 4: (10240, 10280, 10320), 5: (20480, 20560, 20640),
          6: (40880, 41040, 41200), 7: (81680, 82000, 82320)}
# T0 = 4095 (N = 20480, above), 4096, 4097 against the WS_CHUNK = 4096 frames of the moment kernel
CHUNK_N = (20485, 20490)
SEAMS = tuple(n for i in sorted(SEAM_N) for n in SEAM_N[i]) + CHUNK_N
# T of the positional conv's 256-row tile and its 383-row halo, with the smallest N of each
POSCONV_T = {1: 400, 2: 720, 64: 20560, 65: 20880, 128: 41040, 129: 41360, 257: 82320, 320: 102480, 513: 164240}
# conv 0 alone: its 64-frame workgroup, its 16-frame LDS sub-tile and the moment chunk; each T0 at N = 5 T0 + 5 + r, r = 0 (tight) and 3 (residue)
CONV0_T0 = (1, 15, 16, 17, 63, 64, 65, 129, 4097)
CONV0_N = tuple(5 * t0 + 5 + r for t0 in CONV0_T0 for r in (0, 3))

LENGTHS = tuple(sorted(set(SMALL + TIGHT + RESIDUE + SEAMS + tuple(POSCONV_T.values()))))
# ids end to end: SMALL, TIGHT and the L[i] = 256 seam of every conv
IDS_LENGTHS = tuple(sorted(set(SMALL + TIGHT + tuple(SEAM_N[i][1] for i in sorted(SEAM_N)))))

# Which table lengths witness conv i's last USED input row: zeroing that row reaches the final features only when every later conv uses its own last row
# too (it feeds the last output row only). TIGHT does for every conv; the SMALL lengths listed are those whose L[i+1..6] line up.
WITNESS = {1: (400, 720, 1040), 2: (405, 720), 3: (415, 1040), 4: (435, 720), 5: (475, 1040), 6: (555, 720)}
# ... and lengths where conv i has an unused trailing input row (L[i] even for k = 3, odd for k = 2)
SLACK = {1: (405, 415), 2: (410, 415), 3: (420, 425), 4: (440, 445), 5: (480, 485), 6: (560, 565)}


def batch_of(N: int) -> int:
    return 3 if N < 20000 else 2


def waveform(N: int, batch: int = None) -> torch.Tensor:
    """The table's input for length N: normalised float32 [batch, N] (hubert_processor per clip)."""
    from audiotoken_amd.hubert import hubert_processor
    wav = W.synth_waveform(batch_of(N) if batch is None else batch, N, 16000, seed=9000 + N)
    return torch.stack([hubert_processor(torch.from_numpy(r)) for r in wav])


def ragged_mask(N: int, batch: int) -> torch.Tensor:
    """All ones below N = 20000; above, the last clip is valid on its first two thirds only."""
    m = torch.ones(batch, N)
    if N >= 20000:
        m[batch - 1, N * 2 // 3:] = 0
    return m


def weights(n_layers: int = 1):
    return W.synth_hubert_weights(n_layers, WEIGHT_SEED, True)


def _t64(w, key):
    v = w[key]
    v = v if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))
    return v.to(torch.float64)


def conv0_f64(wave, w0, gamma, beta, gn_windows: str = "exact"):
    """conv1d(k 10, stride 5) -> GroupNorm(512 groups, eps 1e-5) -> GELU in float64: [B, N] -> [B, 512, T0].

    gn_windows is the mutant switch of the CPU tests: "exact" = the statistics over the T0 frames; "plus_one" = over T0 + 1 windows, the extra one read
    past the clip's end as zeros (a moment sweep with `t <= T0`); "tail" = the sums include that partial window but are still divided by T0 (a sweep
    bounded by N instead of 5 T0 + 5)."""
    x = wave.to(torch.float64)
    y = F.conv1d(x[:, None], w0, stride=5)
    T0 = y.shape[-1]
    if gn_windows == "exact":
        mean, var = y.mean(-1, keepdim=True), y.var(-1, unbiased=False, keepdim=True)
    else:
        ext = F.conv1d(F.pad(x, (0, 5 * T0 + 10 - x.shape[-1]))[:, None], w0, stride=5)
        assert ext.shape[-1] == T0 + 1
        div = T0 + 1 if gn_windows == "plus_one" else T0
        mean = ext.sum(-1, keepdim=True) / div
        var = (ext * ext).sum(-1, keepdim=True) / div - mean * mean
    y = (y - mean) / torch.sqrt(var + 1e-5) * gamma[None, :, None] + beta[None, :, None]
    return F.gelu(y)


def conv_features_f64(w, wave, edit=None, gn_windows: str = "exact"):
    """The float64 twin of oracle.hubert_ref.conv_features: the same ops in torch.float64. [B, N] -> [B, T, 512].

    edit(i, h) -> h, when given, may change the input [B, 512, L[i]] of conv i = 1..6 (the CPU tests' row mutants)."""
    h = conv0_f64(wave, _t64(w, "feature_extractor.conv_layers.0.conv.weight"), _t64(w, "feature_extractor.conv_layers.0.layer_norm.weight"),
                  _t64(w, "feature_extractor.conv_layers.0.layer_norm.bias"), gn_windows)
    for i in range(1, 7):
        if edit is not None:
            h = edit(i, h)
        h = F.gelu(F.conv1d(h, _t64(w, f"feature_extractor.conv_layers.{i}.conv.weight"), stride=STRIDES[i]))
    return h.transpose(1, 2)


def frame_len(s: int) -> int:
    """Valid frames of a clip whose sample mask sums to s (floor division, so s < 400 gives 0 or less)."""
    for k, st in zip(KERNELS, STRIDES):
        s = (s - k) // st + 1
    return s
