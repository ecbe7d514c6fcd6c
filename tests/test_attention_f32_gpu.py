"""GPU: the fp32 flash attention (csrc/w2vbert_kernels.hip: relpos_attention_kernel) through at_op_attention_f32, against float64
softmax(q k^T / 8 + bias + mask) v — in the form the fine stage launches at every layer (no rel-pos table, heads = E / 64, a mask of ones) and in the
conformer's (distance table, 16 heads, ragged mask; the bias as oracle/w2vbert_ref.relpos_attention forms it, in float64).

The bar is taken from the reference at run time: torch's own fp32 CPU attention on the same inputs errs by e32 against the same float64 result; the kernel
may err by 4 * e32 (another summation order, exp2 in place of exp), never less than n_keys * 2^-24 * max|v| (a convex combination of n_keys terms) and
never more than the 2e-5 tests/test_semantic_gpu.py allows the split-arithmetic kernels.

Largest observed ratio kernel error / torch fp32 error on an MI355X: 1.78 (fine form, 16 heads, T = 1024, B = 3: 9.4e-6 against 5.3e-6); 1.5 the next
largest, 0.7 .. 1.3 for every T <= 700. Every test prints both errors.

Not a case, on purpose: a clip whose keys are ALL padded. The kernel then forms exp2(-inf - -inf); the product never builds such a clip (every clip has a
frame, and the fine stage masks nothing).
"""
import math

import pytest
import torch

from audiotoken_amd import _cabi, prng
from oracle import w2vbert_ref as WR

pytestmark = pytest.mark.gpu

FMIN = torch.finfo(torch.float32).min
CAP = 2e-5
_REF = {}


def _inputs(tag, B, T, heads, scale=1.5):
    hid = heads * 64
    return torch.from_numpy(prng.irwin_hall(f"attn32.{tag}.{B}.{T}.{heads}", (B * T, 3 * hid), 1.0, 7)) * scale


def _dist_table():
    de = torch.zeros(80, 64)
    de[:73] = torch.from_numpy(prng.irwin_hall("attn32.dist", (73, 64), 0.5, 7))
    return de


def _attention(qkv, mask, dist, B, T, heads, dtype):
    """softmax(q k^T / 8 + rel-pos bias + additive finfo.min at padded keys) v in `dtype`, clip by clip; [B * T][heads * 64]."""
    hid = heads * 64
    x = qkv.to(dtype).reshape(B, T, 3, heads, 64)
    out = torch.empty(B, T, hid, dtype=dtype)
    bias_pe = None
    if dist is not None:
        pos = torch.arange(T)
        d = torch.clamp(pos.view(1, -1) - pos.view(-1, 1), -WR.LEFT_MAX, WR.RIGHT_MAX) + WR.LEFT_MAX
        bias_pe = dist.to(dtype)[d]                                         # [T][T][64]
    for b in range(B):
        q, k, v = (x[b, :, i].transpose(0, 1) for i in range(3))            # [heads][T][64]
        logits = (q @ k.transpose(-1, -2)) * 0.125
        if bias_pe is not None:
            logits = logits + torch.einsum("hld,lrd->hlr", q, bias_pe) / math.sqrt(64)
        logits = logits + ((1.0 - mask[b].to(dtype)) * FMIN)[None, None, :]
        out[b] = (torch.softmax(logits, dim=-1) @ v).transpose(0, 1).reshape(T, hid)
    return out.reshape(B * T, hid)


def _reference(key, qkv, mask, dist, B, T, heads):
    """(float64 result, torch fp32 CPU error against it), computed once per input set."""
    if key not in _REF:
        ref = _attention(qkv, mask, dist, B, T, heads, torch.float64)
        e32 = (_attention(qkv, mask, dist, B, T, heads, torch.float32).double() - ref).abs().max().item()
        _REF[key] = (ref, e32)
    return _REF[key]


def _run(dev, qkv_dev, mask, dist, B, T, heads):
    lib = _cabi.load()
    md = mask.reshape(-1).contiguous().to(dev)
    dd = dist.to(dev) if dist is not None else None
    ctx = torch.full((B * T, heads * 64), float("nan"), device=dev)
    _cabi.check(lib.at_op_attention_f32(qkv_dev.data_ptr(), md.data_ptr(), _cabi.ptr(dd), ctx.data_ptr(), B, T, heads,
                                        _cabi.current_stream_handle(dev)), "at_op_attention_f32")
    torch.cuda.synchronize()
    return ctx


def _bar(e32, n_keys, vmax):
    return min(max(4.0 * e32, n_keys * 2.0 ** -24 * vmax), CAP)


def _check(what, got, ref, e32, n_keys, vmax, rows=None):
    got = got.cpu().double()
    if rows is not None:
        got, ref = got[rows], ref[rows]
    assert torch.isfinite(got).all(), f"{what}: non-finite or unwritten outputs"
    err = (got - ref).abs().max().item()
    bar = _bar(e32, n_keys, vmax)
    print(f"{what}: kernel err {err:.3e}, torch fp32 err {e32:.3e}, ratio {err / max(e32, 1e-300):.2f}, bar {bar:.3e}")
    assert err <= bar, f"{what}: error {err:.3e} above the bar {bar:.3e} (torch fp32 errs by {e32:.3e})"


def _vmax(qkv, heads):
    return qkv[:, 2 * heads * 64:].abs().max().item()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("T", [1, 63, 64, 65, 127, 128, 129, 1024])
@pytest.mark.parametrize("heads", [1, 12, 16])
def test_fine_stage_form(cuda_device, heads, T, B):
    """No table, a mask of ones, hid = heads * 64: one key tile, a tile boundary +- 1, two query tiles, and the fine stage's full window."""
    qkv = _inputs("fine", B, T, heads)
    mask = torch.ones(B, T)
    ref, e32 = _reference(("fine", B, T, heads), qkv, mask, None, B, T, heads)
    got = _run(cuda_device, qkv.to(cuda_device), mask, None, B, T, heads)
    _check(f"fine form heads={heads} T={T} B={B}", got, ref, e32, T, _vmax(qkv, heads))


@pytest.mark.parametrize("T", [1, 65, 257])
def test_conformer_form(cuda_device, T):
    """Distance table, 16 heads, a ragged mask (clip 1 padded from two thirds on)."""
    B, heads = 2, 16
    qkv = _inputs("conf", B, T, heads)
    mask = torch.ones(B, T)
    mask[1, max(1, 2 * T // 3):] = 0
    dist = _dist_table()
    ref, e32 = _reference(("conf", T), qkv, mask, dist, B, T, heads)
    got = _run(cuda_device, qkv.to(cuda_device), mask, dist, B, T, heads)
    _check(f"conformer form T={T}", got, ref, e32, T, _vmax(qkv, heads))


def test_masks_without_a_table(cuda_device):
    """A padded tail, padded keys in the interior of a tile, and a key tile that is wholly padded between two live ones."""
    B, T, heads = 3, 200, 12
    qkv = _inputs("mask", B, T, heads)
    mask = torch.ones(B, T)
    mask[0, 150:] = 0
    mask[1, 70:90] = 0
    mask[1, [3, 40, 131, 199]] = 0
    mask[2, 64:128] = 0
    ref, e32 = _reference("mask", qkv, mask, None, B, T, heads)
    got = _run(cuda_device, qkv.to(cuda_device), mask, None, B, T, heads)
    _check("masks", got, ref, e32, T, _vmax(qkv, heads))


def test_spiked_key_in_a_late_tile(cuda_device):
    """Key 400 of T = 700 scaled by 6: the running maximum jumps in tile 6 and the rescale branch runs."""
    B, T, heads = 2, 700, 12
    hid = heads * 64
    qkv = _inputs("spike", B, T, heads)
    qkv[400, hid:hid + 64] *= 6.0
    mask = torch.ones(B, T)
    mask[1, 500:] = 0
    ref, e32 = _reference("spike", qkv, mask, None, B, T, heads)
    got = _run(cuda_device, qkv.to(cuda_device), mask, None, B, T, heads)
    _check("spiked key", got, ref, e32, T, _vmax(qkv, heads))


def test_poisoned_neighbour(cuda_device):
    """The K / V tile loads of keys past T rely on the per-clip buffer descriptor returning zero: a leak from the rows that follow the clip would put
    0 * NaN into P.V. B = 2 with clip 1's rows NaN (clip 0 must be finite and within the bar; clip 1's own output is not examined), and B = 1 with the
    clip at the front of a NaN-filled allocation, so that every row past T is poison too."""
    T, heads = 65, 12
    hid = heads * 64
    qkv = _inputs("poison", 1, T, heads)
    mask1 = torch.ones(1, T)
    ref, e32 = _reference("poison", qkv, mask1, None, 1, T, heads)
    two = torch.full((2 * T, 3 * hid), float("nan"))
    two[:T] = qkv
    got = _run(cuda_device, two.to(cuda_device), torch.ones(2, T), None, 2, T, heads)
    _check("poisoned neighbour, B=2", got, ref, e32, T, _vmax(qkv, heads), rows=slice(0, T))
    buf = torch.full((T + 128, 3 * hid), float("nan"), device=cuda_device)
    buf[:T] = qkv.to(cuda_device)
    got = _run(cuda_device, buf[:T], mask1, None, 1, T, heads)
    _check("poisoned rows past T, B=1", got, ref, e32, T, _vmax(qkv, heads))


def test_ten_repeats_are_bit_identical(cuda_device):
    B, T, heads = 3, 1024, 16
    qkv = _inputs("fine", B, T, heads).to(cuda_device)
    mask = torch.ones(B, T)
    first = _run(cuda_device, qkv, mask, None, B, T, heads)
    for it in range(1, 10):
        assert torch.equal(_run(cuda_device, qkv, mask, None, B, T, heads), first), f"run {it} differs from run 0"
