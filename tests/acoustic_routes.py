"""Route model of the acoustic encoder's length-selected kernel dispatch, and the table of clip lengths that reaches every route.

``enc_route`` (audiotoken_amd/csrc/encodec_plan.h) picks the kernels of ``encodec_encode_impl`` (encodec_encode.hip) from the clip length alone. With L[0] = N and
L[s+1] = ceil(L[s] / (2, 4, 5, 8)[s]) (``make_plan``), five predicates choose the route:

  a  N % 2 == 0                    `fused0`:      seanet_stage0* fused          | conv0_kernel + GEMM block + GEMM strided conv
  b  L[1] % 4 == 0 and L[1] >= 8   `stage1`:      seanet_res64down (or down64*) | seanet_res64* + fp32 windowed GEMM
  c  L[2] % 5 == 0 and L[2] >= 10  `down2_gemm`:  block writes split pieces, reflect_front5, split GEMM | fp32 rows + fp32 GEMM
  d  L[3] % 8 == 0 and L[3] >= 16  with c `chain3`: chained 256-channel block + stage-3 GEMMs; without c the stand-alone
                                   split_phase_major + split GEMM               | GEMM resblock + fp32 strided conv
  e  T = L[4] > 6                  final k = 7 conv as windowed f16x2 split GEMM | zero-extended rows + fp32 conv_gemm (the reference's short-input rule)

(the `fused0`, `stage1_fused`, `down2_gemm`, `chain3` and `down3_gemm` fields of `EncRoute`, and `fin`: `Ty > 6`). All 32 combinations are reachable; N < 321 (L[3] <= 8) is refused.

Plain helper for tests/test_acoustic_routes_cpu.py and tests/test_acoustic_routes_gpu.py — not a conftest, no fixtures.
"""
from audiotoken_amd import weights as W

RATIOS = (2, 4, 5, 8)
MIN_SAMPLES = 321          # the library refuses L[3] <= 8 ("clip too short for the strided convs")
FAMILIES = ("uniform", "trained_like")
B = 3                      # clips per table entry
N_Q = 8                    # bandwidth 6


def chain(N: int):
    """[L[0], ..., L[4]]: the clip length in front of each stage; L[4] = T frames."""
    L = [int(N)]
    for r in RATIOS:
        L.append(-(-L[-1] // r))
    return L


def signature(N: int):
    """(a, b, c, d, e) as 0 / 1, see the module docstring."""
    L = chain(N)
    return (int(N % 2 == 0),
            int(L[1] % 4 == 0 and L[1] >= 8),
            int(L[2] % 5 == 0 and L[2] >= 10),
            int(L[3] % 8 == 0 and L[3] >= 16),
            int(L[4] > 6))


# The smallest N of each of the 32 signatures (T = 2..7; L[1] = 161..1120, L[2] = 41..280, L[3] = 9..56).
SMALL = (321, 322, 327, 328, 353, 354, 359, 360, 601, 602, 607, 608, 633, 634, 639, 640,
         1921, 1922, 1927, 1928, 1953, 1954, 1959, 1960, 2201, 2202, 2207, 2208, 2233, 2234, 2239, 2240)

# One length in 9000..30000 per signature with e = 1, chosen so that a fused kernel ends on a ragged tile: the stage-0 / stage-1 kernels work
# in 64-row tiles, seanet_res128rs in 32-row tiles. L[1] % 64 in {1, 63} and / or L[2] % 32 in {1, 31} where the signature allows it.
# b, c and d together force L[1] = 160 k; an odd k then gives the raggedest tiles there are: L[1] % 64 = 32 and L[2] % 32 in {8, 24}.
MID = (9729,    # (0,0,0,0,1)  L[1] % 64 = 1,  L[2] % 32 = 1
       10229,   # (0,0,0,1,1)  L[1] % 64 = 59, L[2] % 32 = 31
       12033,   # (0,0,1,0,1)  L[1] % 64 = 1,  L[2] % 32 = 1
       13437,   # (0,0,1,1,1)  L[1] % 64 = 63
       14583,   # (0,1,0,0,1)  L[2] % 32 = 31
       16631,   # (0,1,0,1,1)  L[2] % 32 = 31
       17399,   # (0,1,1,0,1)  L[2] % 32 = 31
       22719,   # (0,1,1,1,1)  L[1] % 64 = 32, L[2] % 32 = 24
       18690,   # (1,0,0,0,1)  L[1] % 64 = 1,  L[2] % 32 = 1
       20466,   # (1,0,0,1,1)  L[2] % 32 = 31
       20994,   # (1,0,1,0,1)  L[1] % 64 = 1,  L[2] % 32 = 1
       22398,   # (1,0,1,1,1)  L[1] % 64 = 63
       23816,   # (1,1,0,0,1)  L[2] % 32 = 1
       25592,   # (1,1,0,1,1)  L[2] % 32 = 31
       26360,   # (1,1,1,0,1)  L[2] % 32 = 31
       14400)   # (1,1,1,1,1)  L[1] % 64 = 32, L[2] % 32 = 8

# Padded-row seams of make_plan: T = 256 is the last length whose final-conv operand fits one 256-row pad (Mpf = 256, L[3] = 2048 = Mp2 = Mpc);
# T = 257 steps Mpf to 512 and Mp2 / Mpc to 2304. The odd neighbours have the same L[1..4] behind the unfused stage 0.
SEAMS = (81919, 81920, 82239, 82240)

LENGTHS = SMALL + MID + SEAMS

# Batch-side cross (B = 81, subbatch 2): the all-false signature (fully unfused stack AND the short final conv), the stand-alone split route
# (c false, d true, T = 7) and a T <= 6 length on the fully fused stack (chain3).
BATCH_CROSS = (321, 2202, 633)
BATCH_CROSS_B = 81         # one past kPipeMaxClips
BATCH_CROSS_SUBBATCH = 2


def waveform(N: int, batch: int = B):
    """The table's input for length N: float32 numpy [batch, N]."""
    return W.synth_waveform(batch, N, 24000, seed=7000 + N)


def expected_launches(sig):
    """{profile group: launch count} of the conv stack and the final conv that the signature predicts for ONE sub-batch; a group that must
    not appear maps to 0. (encodec_encode.hip: the prof.begin calls of the stage functions.)"""
    a, b, c, d, e = sig
    chain3 = c and d
    return {
        "stage0_fused": 1 if a else 0,
        "conv0": 0 if a else 1, "res0": 0 if a else 2, "down0": 0 if a else 1,
        "res1_down1": 1 if b else 0,
        "res1": 0 if b else 1, "down1": 0 if b else 1,
        "res2": 2 if c else 1, "down2": 1,
        "res3": 3 if chain3 else 2,
        "down3": 2 if (d and not c) else 1,      # the stand-alone split pass + its GEMM
        "final_conv": 1 if e else 2,             # row copy into the zero-extended buffer + fp32 conv (kernel launches: the memset in front is not counted)
    }


def expected_range_sites(sig):
    """{range-report site: True when it must read > 0 (a split writer of the f16x2 scheme ran there), False when it must read 0.0}.
    `down2` is the stage-2 GEMM's splitting epilogue: it runs with chain3, never without c; with c alone the GEMM's epilogue is linear and the
    site is not part of the evidence (absent from the dict)."""
    a, b, c, d, e = sig
    want = {"res3_conv": bool(c and d), "res3_tail": bool(c and d), "final_conv_in": bool(e)}
    if not c or d:
        want["down2"] = bool(c and d)
    return want
