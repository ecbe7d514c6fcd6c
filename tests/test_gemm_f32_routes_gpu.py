"""GPU: the fp32 windowed GEMM (csrc/gemm_f32.hip, gemm_core.h) on every (tile configuration, body) pair it can take, through at_op_gemm /
at_op_gemm_dual. The table is tests/gemm_f32_cases.py; tests/test_gemm_f32_routes_cpu.py holds every case to the route it claims.

Each case is checked two ways:
 (a) against the float64 contraction, with the per-element bar gemm_f32_cases.reference derives from the operands (an fp32 FMA chain's error bound
     plus the measured allowance of the approximated activation), never looser than tests/test_ops_gpu.py's 1.6e-4 * max|ref|;
 (b) bit for bit against the same rows computed as a plain Linear (ktaps == 1, at most 64 rows per launch: the 64x64 or a narrow configuration) over a
     host-built im2col matrix — the k order is the same on every configuration and body, and zero-filled K tails add exact zeros. PRO_POWER has no
     im2col form; its partner is the same launch with fewer columns (another body for the last n-tile, or another configuration).
Outputs are prefilled with NaN: every element must be written, and columns between N and ldc must stay NaN.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from tests import gemm_f32_cases as G

pytestmark = pytest.mark.gpu

_HOST = {}     # case name -> (tensors, ref, bar): the float64 reference is computed once per case
_OUT = {}      # case name -> output of the case's launch (CPU tensor [batch][M][ldc])


def _host(c):
    if c.name not in _HOST:
        t = G.build(c)
        _HOST[c.name] = (t, *G.reference(c, t))
    return _HOST[c.name]


def _launch(c, tensors, dev, N=None, out=None):
    """One at_op_gemm / at_op_gemm_dual call for case c over host tensors (numpy); returns the device output [batch][M][ldc] (NaN-prefilled unless given)."""
    lib = _cabi.load()
    td = {k: torch.from_numpy(np.ascontiguousarray(v)).to(dev) for k, v in tensors.items()}
    if out is None:
        out = torch.full((c.batch, c.M, c.c_ld), float("nan"), dtype=torch.float32, device=dev)
    ptrs = {k: v.data_ptr() for k, v in td.items()}
    ptrs["C"] = out.data_ptr()
    if c.residual == "inplace":
        ptrs["R"] = out.data_ptr()
    d = G.fill_desc(_cabi.GemmDesc(), c, ptrs, N=N)
    st = _cabi.current_stream_handle(dev)
    if c.K2:
        _cabi.check(lib.at_op_gemm_dual(C.byref(d), *G.dual_args(c, ptrs), st), "at_op_gemm_dual")
    else:
        _cabi.check(lib.at_op_gemm(C.byref(d), st), "at_op_gemm")
    torch.cuda.synchronize()
    return out


def _run(c, dev):
    if c.name not in _OUT:
        t = _host(c)[0]
        if c.residual == "inplace":
            # R == C: the output starts as the residual. Every element is still proven written: the result must equal, bit for bit, the same launch with
            # the residual in a tensor of its own and a NaN-prefilled output
            sep = _launch(G.replace(c, residual="sep"), t, dev)
            out = _launch(c, {k: v for k, v in t.items() if k != "R"}, dev, out=torch.from_numpy(t["R"].copy()).to(dev))
            assert not torch.isnan(sep).any()
            assert torch.equal(out, sep), f"{c.name}: the in-place residual differs from the separate one"
        else:
            out = _launch(c, t, dev)
        _OUT[c.name] = out.cpu()
    return _OUT[c.name]


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case_vs_float64(cuda_device, c):
    t, ref, bar = _host(c)
    out = _run(c, cuda_device)
    n = c.n_out
    got = out[:, :, :n].numpy().astype(np.float64)
    assert not np.isnan(got).any(), f"{c.name}: {int(np.isnan(got).sum())} outputs not written"
    if c.c_ld > n:
        assert torch.isnan(out[:, :, n:]).all(), f"{c.name}: columns between N and ldc were written"
    err = np.abs(got - ref)
    worst = np.unravel_index(np.argmax(err - bar), err.shape)
    print(f"{c.name}: max err {err.max():.3e}, largest err / bar {np.max(err / np.maximum(bar, 1e-300)):.3f}, bar at the worst element {bar[worst]:.3e}, "
          f"legacy bar {G.LEGACY_TOL * np.abs(ref).max():.3e}")
    if c.row_mask:
        masked = t["mask"] == 0
        assert masked.any() and np.all(got[masked] == 0.0), f"{c.name}: masked rows must be exact zeros"
    assert np.all(err <= bar), f"{c.name}: element {worst} errs by {err[worst]:.3e}, bar {bar[worst]:.3e} (ref {ref[worst]:.6e})"


def _twin_chunk(c, t, dev, b, rows):
    """Rows `rows` of clip b as a plain Linear over the host-built A: the same weights, bias, prologue, epilogue, alpha, residual and mask."""
    a = G.im2col(c, t, b, rows)
    k1 = c.Cin if c.K2 else c.K
    tw = G.Case("twin", (), M=len(rows), N=c.N, Cin=k1, K2=c.K2, ld2=c.K2, pro=c.pro, epi=c.epi, alpha=c.alpha, bias=c.bias,
                residual="sep" if c.residual else "", row_mask=c.row_mask)
    tt = {"X": a[None, :, :k1], "W": t["W"]}
    if c.K2:
        tt["X2"] = a[None, :, k1:]
    if c.bias:
        tt["bias"] = t["bias"]
    if c.residual:
        tt["R"] = t["R"][b][rows, :c.n_out][None]
    if c.row_mask:
        tt["mask"] = t["mask"][b][rows][None]
    return _launch(tw, tt, dev)[0].cpu()


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case_bit_identical_to_plain_linear(cuda_device, c):
    t = _host(c)[0]
    out = _run(c, cuda_device)
    n = c.n_out
    if c.pro == G.PRO_POWER:
        twin = _launch(c, t, cuda_device, N=c.twin_N).cpu()
        assert not torch.isnan(twin[:, :, :c.twin_N]).any() and torch.isnan(twin[:, :, c.twin_N:]).all()
        diff = (twin[:, :, :c.twin_N] != out[:, :, :c.twin_N])
        assert not diff.any(), f"{c.name}: {int(diff.sum())} of the first {c.twin_N} columns differ between N = {c.N} and N = {c.twin_N}"
        return
    bad = 0
    for b, r0, r1 in G.twin_rows(c):
        for s in range(r0, r1, 64):
            rows = np.arange(s, min(s + 64, r1))
            twin = _twin_chunk(c, t, cuda_device, b, rows)
            assert not torch.isnan(twin).any()
            diff = twin != out[b, s:s + len(rows), :n]
            if diff.any():
                bad += int(diff.sum())
                i = torch.nonzero(diff)[0].tolist()
                print(f"{c.name}: clip {b} rows {s}..{s + len(rows) - 1}: {int(diff.sum())} elements differ, first at row {s + i[0]} column {i[1]}: "
                      f"{out[b, s + i[0], i[1]].item()!r} vs the Linear's {twin[i[0], i[1]].item()!r}")
    assert bad == 0, f"{c.name}: {bad} elements differ from the plain Linear over im2col rows"


def test_soak_largest_k16_case_is_bit_stable(cuda_device):
    """The double-buffered LDS staging has no atomics: any run-to-run difference is a race."""
    c = G.BY_NAME[G.SOAK]
    t = _host(c)[0]
    first = _run(c, cuda_device).to(cuda_device)
    td = {k: torch.from_numpy(v).to(cuda_device) for k, v in t.items()}
    lib = _cabi.load()
    for it in range(1, 10):
        out = torch.full((c.batch, c.M, c.c_ld), float("nan"), dtype=torch.float32, device=cuda_device)
        ptrs = {k: v.data_ptr() for k, v in td.items()}
        ptrs["C"] = out.data_ptr()
        d = G.fill_desc(_cabi.GemmDesc(), c, ptrs)
        _cabi.check(lib.at_op_gemm(C.byref(d), _cabi.current_stream_handle(cuda_device)), "at_op_gemm")
        torch.cuda.synchronize()
        assert torch.equal(out, first), f"run {it} differs from run 0"


def _probe(dev, x, pro, epi):
    """f(x) as the kernel computes it: identity weights make the pre-activation the fp32 input itself (x * 1 plus exact zeros), so the whole error of the
    output is the approximated function's."""
    n = x.shape[1]
    c = G.Case("probe", (), M=x.shape[0], N=n, Cin=n, pro=pro, epi=epi, bias=False)
    return _launch(c, {"X": x[None], "W": np.eye(n, dtype=np.float32)}, dev)[0].cpu().numpy().astype(np.float64)


def test_activation_allowances(cuda_device):
    """The allowances in gemm_f32_cases.ALLOW / ALLOW_PRO_ELU against what the hardware's v_exp_f32 / v_rcp_f32 / logf forms actually deliver:
    observed error in ulps of max(|out|, 1) against the float64 function, over [-12, 12] plus a dense band around zero (log: 1e-9 .. 50 and zeros)."""
    from audiotoken_amd import prng
    x = prng.uniform("probe.x", (1024, 128), -12.0, 12.0, seed=5)
    x[::4] = prng.uniform("probe.x0", (256, 128), -1.0, 1.0, seed=5)
    x[1::16] *= np.float32(1e-3)
    x[0, :8] = [0.0, -0.0, 1.0, -1.0, 88.0, -88.0, -104.0, 1e-30]
    x64 = x.astype(np.float64)
    seen = {}
    for epi in (G.EPI_SWISH, G.EPI_ELU, G.EPI_GELU):
        want = G.activation64(epi, x64)
        seen[epi] = np.max(np.abs(_probe(cuda_device, x, G.PRO_NONE, epi) - want) / G.ulp1(want))
    want = G.activation64(G.EPI_GLU, x64)
    seen[G.EPI_GLU] = np.max(np.abs(_probe(cuda_device, x, G.PRO_NONE, G.EPI_GLU) - want) / G.ulp1(want))
    p = np.exp(prng.uniform("probe.p", (1024, 128), -20.0, 4.0, seed=5).astype(np.float64)).astype(np.float32)
    p[::9, ::3] = 0.0
    p[1, :4] = [G.LOG_FLOOR, np.float32(G.LOG_FLOOR) * np.float32(0.999), 1.0, np.nextafter(np.float32(1.0), np.float32(2.0))]
    want = G.activation64(G.EPI_LOGFLOOR, p.astype(np.float64))
    seen[G.EPI_LOGFLOOR] = np.max(np.abs(_probe(cuda_device, p, G.PRO_NONE, G.EPI_LOGFLOOR) - want) / G.ulp1(want))
    pro = np.max(np.abs(_probe(cuda_device, x, G.PRO_ELU, G.EPI_NONE) - G.activation64(G.EPI_ELU, x64))[x64 <= 0]) / G.U
    names = {G.EPI_SWISH: "swish", G.EPI_ELU: "ELU", G.EPI_GELU: "GELU", G.EPI_GLU: "GLU", G.EPI_LOGFLOOR: "log floor"}
    for epi, v in seen.items():
        print(f"epilogue {names[epi]}: observed {v:.3f} ulp, allowance {G.ALLOW[epi]}")
    print(f"prologue ELU: observed {pro:.3f} units of 2^-24, allowance {G.ALLOW_PRO_ELU}")
    for epi, v in seen.items():
        assert v <= G.ALLOW[epi], f"{names[epi]}: {v:.3f} ulp observed, {G.ALLOW[epi]} allowed"
    assert pro <= G.ALLOW_PRO_ELU
    # ELU touches the first source only, and positive inputs pass through the prologue untouched
    assert np.array_equal(_probe(cuda_device, x, G.PRO_ELU, G.EPI_NONE)[x64 > 0], x64[x64 > 0])
