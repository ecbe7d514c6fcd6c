"""Route model of the fp32 windowed GEMM (audiotoken_amd/csrc/gemm_f32.hip, gemm_core.h) and the table of shapes that reaches every route.

``launch_gemm`` picks one of seven tile configurations from the shape (``gemm_config``); each workgroup then picks one of three bodies
(``gemm_body``: FAST, TAP, general). ``at_op_gemm_route`` reports both without launching anything. Derived from the two predicates
(RPP = rows staged per pass = 32 for a K tile of 32, 64 for a K tile of 16; FAST and TAP need BN >= RPP), the reachable (configuration, body) pairs are

  128x16               general only: BN = 16 < RPP = 32
  128x32, 128x64,      FAST, TAP and general each (general: K % 32 != 0, or ktaps > 1 with Cin % 32 != 0, or a second source with K1 % 32 != 0)
  64x64, 128x128
  128x128 K tile 16    all three: the configuration needs pro == NONE and K % 16 == 0; general then needs ktaps > 1 with Cin % 16 != 0 (or a second
                       source with K1 % 16 != 0)
  128x64 K tile 16     FAST and TAP only: chosen only for ktaps > 1 with Cin % 16 == 0 and K % 16 == 0, so the TAP predicate always holds

18 pairs: REACHABLE below. This is the list the issue that asked for these tests arrived at; the code agrees.
tests/test_gemm_f32_routes_cpu.py holds every case to the pairs it claims, tests/test_gemm_f32_routes_gpu.py runs the cases.

The contraction every case states (csrc/at_common.h):
  out[b][m][n] = alpha * epi( sum_kk A(b,m,kk) W[n][kk] + bias[n] ) + R[b][m][n],   rows with row_mask 0 written as 0
  A(b,m,kk) = pro( X[b][m*stride + kk/Cin - pad_left][kk % Cin] ), rows outside [0, Tin) reflected (pad_mode 1) or zero (pad_mode 0);
  with a second source (ktaps == 1): A = [ pro(X[b][m][:K1]) | X2[b][m][:K - K1] ];  EPI_GLU: out[m][c] = v[2c] * sigmoid(v[2c + 1]), no alpha / R.

Plain helper module — not a conftest, no fixtures.
"""
from dataclasses import dataclass, replace

import numpy as np

from audiotoken_amd import prng

# configuration ids (csrc/at_common.h: GemmConfig) and body ids (csrc/gemm_core.h: GemmBody): at_op_gemm_route's out[0] and the index into out[1:4]
C128x16, C128x32, C128x64, C128x64_K16, C64x64, C128x128_K16, C128x128 = range(7)
GENERAL, FAST, TAP = 0, 1, 2
CONFIG_NAMES = ("128x16", "128x32", "128x64", "128x64/K16", "64x64", "128x128/K16", "128x128")
BODY_NAMES = ("general", "FAST", "TAP")
REACHABLE = frozenset(
    [(C128x16, GENERAL)]
    + [(c, b) for c in (C128x32, C128x64, C64x64, C128x128, C128x128_K16) for b in (GENERAL, FAST, TAP)]
    + [(C128x64_K16, FAST), (C128x64_K16, TAP)])

PRO_NONE, PRO_ELU, PRO_POWER = 0, 1, 2
EPI_NONE, EPI_SWISH, EPI_ELU, EPI_GELU, EPI_LOGFLOOR, EPI_GLU = range(6)
LOG_FLOOR = 1.192092955078125e-07   # 2^-23, the mel floor of EPI_LOGFLOOR
U = 2.0 ** -24                      # unit roundoff of fp32

MAX_OUT_BYTES = 16 << 20
MAX_K = 192


@dataclass(frozen=True)
class Case:
    name: str
    routes: tuple           # the (configuration, body) pairs the case is in the table for
    M: int
    N: int
    Cin: int
    ktaps: int = 1
    stride: int = 1
    pad_left: int = 0
    pad_mode: int = 0
    Tin: int = 0            # 0 = M
    batch: int = 1
    ldx: int = 0            # floats between input rows (0 = Cin); x_off = column of the op's first channel inside such a row
    x_off: int = 0
    K2: int = 0             # width of the second source (0 = single source), ld2 its row stride
    ld2: int = 0
    pro: int = PRO_NONE
    aux_off: int = 0
    epi: int = EPI_NONE
    alpha: float = 1.0
    bias: bool = True
    residual: str = ""      # "" none, "sep" a separate tensor, "inplace" R == C
    row_mask: bool = False
    ldc: int = 0            # 0 = N (N / 2 for EPI_GLU)
    twin_N: int = 0         # PRO_POWER only: the N of the twin launch that computes the same leading columns on another body

    @property
    def K(self):
        return self.ktaps * self.Cin + self.K2

    @property
    def tin(self):
        return self.Tin or self.M

    @property
    def x_ld(self):
        return self.ldx or self.Cin

    @property
    def n_out(self):
        return self.N // 2 if self.epi == EPI_GLU else self.N

    @property
    def c_ld(self):
        return self.ldc or self.n_out

    @property
    def out_bytes(self):
        return self.batch * self.M * self.c_ld * 4


_BIG = dict(M=1040, N=3712)     # 9 x 29 = 261 tiles of 128 x 128 and M * batch > 1024: the smallest launch that leaves the 64 x 64 configuration

CASES = (
    # ---- 128x128, K tile 16 (pro NONE, K % 16 == 0): the product's full-batch shape ---------------------------------------------------------
    Case("big16_fast", ((C128x128_K16, FAST),), **_BIG, Cin=48),
    Case("big16_ntail", ((C128x128_K16, TAP), (C128x128_K16, FAST)), M=1040, N=3716, Cin=48),
    # Cin = 8 < K tile: no K tile lies inside one tap -> general at the zero-padded first m-tile, FAST inside
    Case("big16_conv_cin8", ((C128x128_K16, GENERAL), (C128x128_K16, FAST)), **_BIG, Cin=8, ktaps=2, pad_left=1, Tin=1040),
    # the same size through the batch: x / c / r batch strides, an M tail of 2 rows in every clip, swish, alpha and a residual
    Case("big16_batch8", ((C128x128_K16, FAST),), M=130, N=3712, Cin=48, batch=8, epi=EPI_SWISH, alpha=0.5, residual="sep"),
    # ---- 128x128, K tile 32 (a prologue, or K % 16 != 0) ---------------------------------------------------------------------------------------
    Case("big32_elu_ntail", ((C128x128, FAST), (C128x128, TAP)), M=1040, N=3716, Cin=64, pro=PRO_ELU),
    Case("big32_k40_gelu", ((C128x128, GENERAL),), **_BIG, Cin=40, epi=EPI_GELU),
    Case("big32_power_log", ((C128x128, FAST),), **_BIG, Cin=64, ldx=128, aux_off=64, pro=PRO_POWER, epi=EPI_LOGFLOOR, bias=False, twin_N=3708),
    # ---- 128x64, K tile 16: HuBERT's grouped positional conv (48 channels per group) ---------------------------------------------------------------
    Case("g48_n48_zero", ((C128x64_K16, TAP),), M=300, N=48, Cin=48, ktaps=3, pad_left=1, pad_mode=0),
    Case("g48_n48_reflect", ((C128x64_K16, TAP),), M=300, N=48, Cin=48, ktaps=3, pad_left=1, pad_mode=1),
    Case("g48_n64_zero", ((C128x64_K16, FAST), (C128x64_K16, TAP)), M=300, N=64, Cin=48, ktaps=3, pad_left=1, pad_mode=0),
    Case("g48_n64_reflect", ((C128x64_K16, FAST), (C128x64_K16, TAP)), M=300, N=64, Cin=48, ktaps=3, pad_left=1, pad_mode=1),
    # the grouped form: group 1 of 2 read from rows of 96 floats at column 48 — rows are not contiguous windows, never FAST
    Case("g48_grouped", ((C128x64_K16, TAP),), M=300, N=64, Cin=48, ktaps=3, pad_left=1, pad_mode=0, ldx=96, x_off=48, batch=2),
    # ---- 64x64: launches too small for 128 x 128 tiles ----------------------------------------------------------------------------------------------
    Case("s64_tails", ((C64x64, FAST), (C64x64, TAP)), M=70, N=68, Cin=160, ldc=72),
    Case("dual_tap", ((C64x64, TAP),), M=70, N=68, Cin=32, K2=64, ld2=72, batch=2),
    Case("dual_tap_elu", ((C64x64, TAP),), M=70, N=68, Cin=32, K2=64, ld2=72, batch=2, pro=PRO_ELU),
    # K1 = 16: the first K tile of 32 straddles the two sources
    Case("dual_general", ((C64x64, GENERAL),), M=70, N=68, Cin=16, K2=32, ld2=40, batch=2),
    Case("dual_general_elu", ((C64x64, GENERAL),), M=70, N=68, Cin=16, K2=32, ld2=40, batch=2, pro=PRO_ELU),
    # EPI_GLU: interleaved weight rows, ldc = N / 2, float2 stores; with and without a row mask
    Case("glu", ((C64x64, FAST),), M=200, N=128, Cin=64, batch=2, epi=EPI_GLU),
    Case("glu_masked", ((C64x64, FAST),), M=200, N=128, Cin=64, batch=2, epi=EPI_GLU, row_mask=True),
    # ---- the narrow configurations ---------------------------------------------------------------------------------------------------------------
    Case("n32_k64_ldx", ((C128x32, FAST),), M=200, N=32, Cin=64, ldx=72, x_off=4),        # an M tail in the FAST body; ldx != Cin
    Case("n20_k64", ((C128x32, TAP),), M=200, N=20, Cin=64, ldc=32),
    Case("n32_k48", ((C128x32, GENERAL),), M=200, N=32, Cin=48),
    Case("n64_k64_inplace", ((C128x64, FAST),), M=200, N=64, Cin=64, residual="inplace"),
    Case("n48_k64", ((C128x64, TAP),), M=200, N=48, Cin=64),
    Case("n64_k36", ((C128x64, GENERAL),), M=200, N=64, Cin=36),
    Case("n16_k64", ((C128x16, GENERAL),), M=200, N=16, Cin=64),
    Case("n12_k36", ((C128x16, GENERAL),), M=200, N=12, Cin=36, ldc=16),
    # strided convs whose right edge leaves the clip (Tin is not a multiple of the stride), one per pad mode
    Case("conv_reflect_right", ((C128x32, TAP),), M=101, N=32, Cin=32, ktaps=4, stride=2, pad_left=2, pad_mode=1, Tin=201, batch=2),
    Case("conv_zero_right", ((C128x64, TAP),), M=101, N=64, Cin=32, ktaps=4, stride=2, pad_left=2, pad_mode=0, Tin=201, batch=2),
    # Tin = pad_left + 1: the smallest clip the argument check admits; both ends reflect inside one window
    Case("conv_min_clip", ((C128x16, GENERAL),), M=2, N=16, Cin=32, ktaps=4, stride=2, pad_left=2, pad_mode=1, Tin=3),
    # ktaps > 1 with Cin % 32 != 0 (and % 16 != 0): no K tile inside one tap
    Case("conv_cin12", ((C128x64, GENERAL),), M=200, N=64, Cin=12, ktaps=3, pad_left=2, pad_mode=1, batch=2),
    # ---- prologues and epilogues, once each on the cheapest configuration ------------------------------------------------------------------------
    Case("power_fast_log", ((C128x64, FAST),), M=200, N=64, Cin=64, ldx=128, aux_off=64, pro=PRO_POWER, epi=EPI_LOGFLOOR, bias=False, twin_N=60),
    Case("power_general_log", ((C128x64, GENERAL),), M=200, N=64, Cin=36, ldx=72, aux_off=36, pro=PRO_POWER, epi=EPI_LOGFLOOR, bias=False, twin_N=32),
    Case("rowmask_elu", ((C128x32, FAST),), M=200, N=32, Cin=64, epi=EPI_ELU, row_mask=True, batch=2),
    Case("alpha_res_gelu", ((C128x32, TAP),), M=200, N=20, Cin=64, epi=EPI_GELU, alpha=0.5, residual="sep"),
    Case("swish_res_batch", ((C128x64, FAST),), M=130, N=64, Cin=64, epi=EPI_SWISH, alpha=2.0, residual="sep", batch=3),
)
BY_NAME = {c.name: c for c in CASES}
SOAK = "big16_fast"    # the largest 128x128 K-tile-16 case: 10 bit-identical repeats

# ---- allowances of the approximated functions, MEASURED on an MI355X ------------------------------------------------------------------------------
# Unit: one ulp of the output, 2^-24 * max(|out|, 1). The magnitude is floored at 1 because ELU (v_exp_f32 minus one) and GELU (Abramowitz-Stegun erfc)
# are absolute-accurate by design (csrc/at_common.h: "NOT relative-accurate near 0"): in ulps of an output near zero their error has no bound.
# Measured by test_activation_allowances (identity weights: the pre-activation is the fp32 input itself, so the whole error is the function's) against
# the float64 function; the constant is twice the largest observed value, rounded up to a power of two.
ALLOW = {
    EPI_NONE: 0.0,
    EPI_SWISH: 8.0,      # observed 2.329 ulp   (x * v_rcp_f32(1 + v_exp_f32(-x)))
    EPI_ELU: 4.0,        # observed 1.084 ulp   (v_exp_f32(x) - 1)
    EPI_GELU: 8.0,       # observed 3.601 ulp   (Abramowitz-Stegun 7.1.26 erfc)
    EPI_LOGFLOOR: 8.0,   # observed 2.608 ulp   (logf)
    EPI_GLU: 8.0,        # observed 3.313 ulp   (a * sigmoid(b))
}
ALLOW_PRO_ELU = 4.0      # observed 1.084: absolute, in units of 2^-24 per A element (|ELU| <= 1 on the approximated branch)
LIPSCHITZ = {EPI_NONE: 1.0, EPI_SWISH: 1.1, EPI_ELU: 1.0, EPI_GELU: 1.13}   # sup |f'|: swish 1.0998, GELU 1.1290
LEGACY_TOL = 1.6e-4     # tests/test_ops_gpu.py::_close allows 2e-5 * 8 * max|ref|: no bar here may exceed it


# ---- builders ---------------------------------------------------------------------------------------------------------------------------------------
def build(c: Case):
    """The case's host tensors (numpy float32): X [batch][Tin][ldx], X2 [batch][M][ld2], W [N][K], bias [N], R [batch][M][ldc], mask [batch][M]."""
    t = {}
    if c.pro == PRO_POWER:
        # a spectrum: ordinary rows, rows small enough for every sum to fall below the floor 2^-23, and rows that are exactly zero
        x = prng.uniform(c.name + ".x", (c.batch, c.tin, c.x_ld), -1.0, 1.0, seed=3)
        x[:, 3::7] *= np.float32(1e-5)
        x[:, 5::11] = 0.0
        t["W"] = prng.uniform(c.name + ".w", (c.N, c.K), 0.0, 0.1, seed=3)      # mel filters are non-negative
    else:
        x = prng.uniform(c.name + ".x", (c.batch, c.tin, c.x_ld), -2.0, 2.0, seed=3)
        t["W"] = prng.uniform(c.name + ".w", (c.N, c.K), -0.2, 0.2, seed=3)
    t["X"] = x
    if c.K2:
        t["X2"] = prng.uniform(c.name + ".x2", (c.batch, c.M, c.ld2), -2.0, 2.0, seed=3)
    if c.bias:
        t["bias"] = prng.uniform(c.name + ".b", (c.N,), -1.0, 1.0, seed=3)
    if c.residual:
        t["R"] = prng.uniform(c.name + ".r", (c.batch, c.M, c.c_ld), -1.0, 1.0, seed=3)
    if c.row_mask:
        m = np.ones((c.batch, c.M), dtype=np.float32)
        m[:, 1::5] = 0.0
        m[-1, c.M - 3:] = 0.0
        t["mask"] = m
    return t


def window_rows(c: Case, m):
    """For output rows m (array): (input row, valid) per tap, [len(m)][ktaps] — the reflect / zero rule of the contraction."""
    m = np.asarray(m)
    r = m[:, None] * c.stride + np.arange(c.ktaps)[None, :] - c.pad_left
    last = c.tin - 1
    outside = (r < 0) | (r > last)
    r = np.where(r < 0, -r, np.where(r > last, 2 * last - r, r))
    r = np.clip(r, 0, last)
    return r, (~outside) | (c.pad_mode != 0)


def im2col(c: Case, t, b, m):
    """Raw A rows of clip b for output rows m, [len(m)][K] float32: the windows gathered with the padding applied (zero rows stay zero: ELU(0) = 0),
    the second source appended. The prologue is NOT applied (PRO_POWER cannot be expressed this way: it reads two columns per element)."""
    assert c.pro != PRO_POWER
    r, ok = window_rows(c, m)
    x = t["X"][b][:, c.x_off:c.x_off + c.Cin]
    a = x[r] * ok[:, :, None].astype(np.float32)                 # [rows][ktaps][Cin]
    a = a.reshape(len(m), c.ktaps * c.Cin)
    if c.K2:
        a = np.concatenate([a, t["X2"][b][np.asarray(m), :c.K2]], axis=1)
    return np.ascontiguousarray(a, dtype=np.float32)


def operand64(c: Case, t, b):
    """A of clip b in float64 after the prologue, [M][K], and the mask of elements that went through the ELU prologue's approximated branch."""
    m = np.arange(c.M)
    if c.pro == PRO_POWER:
        x = t["X"][b].astype(np.float64)
        a = x[:c.M, c.x_off:c.x_off + c.Cin] ** 2 + x[:c.M, c.x_off + c.aux_off:c.x_off + c.aux_off + c.Cin] ** 2
        return a, np.zeros_like(a, dtype=bool)
    a = im2col(replace(c, K2=0), t, b, m).astype(np.float64)
    approx = np.zeros_like(a, dtype=bool)
    if c.pro == PRO_ELU:
        approx = a < 0
        a = np.where(a > 0, a, np.expm1(np.minimum(a, 0.0)))
    if c.K2:
        x2 = t["X2"][b][:, :c.K2].astype(np.float64)
        a = np.concatenate([a, x2], axis=1)
        approx = np.concatenate([approx, np.zeros_like(x2, dtype=bool)], axis=1)
    return a, approx


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _erf(x):
    import torch
    return torch.special.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def activation64(epi, v):
    if epi == EPI_SWISH:
        return v * _sigmoid(v)
    if epi == EPI_ELU:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    if epi == EPI_GELU:
        return 0.5 * v * (1.0 + _erf(v / np.sqrt(2.0)))
    if epi == EPI_LOGFLOOR:
        return np.log(np.maximum(v, LOG_FLOOR))
    if epi == EPI_GLU:
        return v[..., 0::2] * _sigmoid(v[..., 1::2])
    return v


def ulp1(out):
    return U * np.maximum(np.abs(out), 1.0)


def reference(c: Case, t):
    """(ref, bar), both float64 [batch][M][n_out]: the contraction in float64 and the per-element error bar of a correct fp32 kernel.

    Before the activation the bar is derived: a k-ordered fp32 FMA chain of length K plus the bias add errs by at most (K + 1) 2^-24 (sum_k |A||W| + |bias|).
    PRO_POWER forms A = fma(x, x, y * y) in fp32 (two roundings, relative): K + 3 in place of K + 1. The ELU prologue errs by at most ALLOW_PRO_ELU 2^-24
    per negative element, times |W|. The activation multiplies the bar by its Lipschitz constant (log: 1 / max(v - bar, floor); GLU: sigmoid(b) for the
    value and |a| / 4 for the gate) and adds its measured allowance. alpha and the residual add one rounding each. Never above LEGACY_TOL * max|ref|."""
    W = t["W"].astype(np.float64)
    refs, bars = [], []
    for b in range(c.batch):
        a, approx = operand64(c, t, b)
        pre = a @ W.T
        mag = np.abs(a) @ np.abs(W).T
        if c.bias:
            pre = pre + t["bias"].astype(np.float64)
            mag = mag + np.abs(t["bias"].astype(np.float64))
        bar = (c.K + 1 + (2 if c.pro == PRO_POWER else 0)) * U * mag
        if c.pro == PRO_ELU:
            bar = bar + ALLOW_PRO_ELU * U * (approx.astype(np.float64) @ np.abs(W).T)
        act = activation64(c.epi, pre)
        if c.epi == EPI_LOGFLOOR:
            bar = bar / np.maximum(pre - bar, LOG_FLOOR)
        elif c.epi == EPI_GLU:
            bar = bar[..., 0::2] * _sigmoid(pre[..., 1::2]) + np.abs(pre[..., 0::2]) * 0.25 * bar[..., 1::2]
        else:
            bar = bar * LIPSCHITZ[c.epi]
        bar = bar + ALLOW[c.epi] * ulp1(act)
        out = act
        if c.epi != EPI_GLU:
            out = act * float(np.float32(c.alpha))
            bar = bar * abs(c.alpha)
            if c.alpha != 1.0:
                bar = bar + U * np.abs(out)
            if c.residual:
                out = out + t["R"][b][:, :c.N].astype(np.float64)
                bar = bar + U * np.abs(out)
        if c.row_mask:
            keep = t["mask"][b][:, None] != 0
            out = np.where(keep, out, 0.0)
            bar = np.where(keep, bar, 0.0)
        refs.append(out)
        bars.append(bar)
    ref, bar = np.stack(refs), np.stack(bars)
    return ref, np.minimum(bar, LEGACY_TOL * np.abs(ref).max())


def twin_rows(c: Case):
    """(clip, first row, last row + 1) ranges compared bit for bit with the plain-Linear twin: every row of the small cases; of a 128 x 128 case the
    first, the last and two interior m-tiles (single clip), or every row of the first and the last clip (batched)."""
    if c.routes[0][0] not in (C128x128, C128x128_K16):
        return [(b, 0, c.M) for b in range(c.batch)]
    if c.batch > 1:
        return [(0, 0, c.M), (c.batch - 1, 0, c.M)]
    last = (c.M - 1) // 128 * 128
    return [(0, 0, 128), (0, 384, 512), (0, 640, 768), (0, last, c.M)]


def fill_desc(d, c: Case, ptrs, N=None):
    """Fill a ``_cabi.GemmDesc`` for the case from a dict of addresses (X, W, bias, C, R, mask; 0 = NULL). N: the twin launch's narrower N."""
    n = N or c.N
    d.X, d.x_bstride, d.Tin, d.Cin, d.ldx = ptrs["X"] + 4 * c.x_off if ptrs["X"] else 0, c.tin * c.x_ld, c.tin, c.Cin, c.x_ld
    d.ktaps, d.stride, d.pad_left, d.pad_mode = c.ktaps, c.stride, c.pad_left, c.pad_mode
    d.W, d.bias = ptrs["W"], ptrs.get("bias", 0)
    d.C, d.c_bstride, d.ldc = ptrs["C"], c.M * c.c_ld, c.c_ld
    d.R, d.r_bstride, d.ldr = ptrs.get("R", 0), c.M * c.c_ld, c.c_ld
    d.M, d.N, d.K, d.batch, d.pro, d.epi, d.alpha = c.M, n, c.K, c.batch, c.pro, c.epi, c.alpha
    d.aux_off, d.row_mask = c.aux_off, ptrs.get("mask", 0)
    return d


def dual_args(c: Case, ptrs):
    """(X2, x2_bstride, ld2, K1) of at_op_gemm_dual / at_op_gemm_route."""
    return (ptrs.get("X2", 0), c.M * c.ld2, c.ld2, c.Cin) if c.K2 else (0, 0, 0, 0)
