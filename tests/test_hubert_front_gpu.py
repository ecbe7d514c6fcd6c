"""GPU: the semantic_s (HuBERT) front end — hub_wavstats / hub_gn_coeff / hub_conv0_gn_gelu, the six strided convs as windowed phase-major split GEMMs (or
fp32 windowed GEMMs), hub_frame_mask and the positional conv — at every length class of tests/hubert_front_cases.py, against float64.

 (a) at_hubert_features (the product's own feature_extractor(), NaN-filled workspace and output) against the float64 twin, bar = c * e_ref with e_ref the
     torch-CPU fp32 oracle's own distance from float64 on the same case (hubert_front_cases.C_BAR);
 (b) at_op_hub_conv0 alone against float64 conv1d + group_norm + gelu on six kinds of waveform, same rule;
 (c) at_op_hub_frame_mask against oracle.hubert_ref.frame_mask, exactly;
 (d) ids of a one-layer model against the oracle (equal, or an oracle near-tie), one clip of a batch with no valid frame;
 (e) hidden state 0 at the positional conv's tile and halo seams on both of its kernels.
tests/test_hubert_front_cpu.py shows that the twin and the bar see the faults these lengths are aimed at. Measured ratios: profiles/hubert_front.txt.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from audiotoken_amd import _cabi
from oracle import hubert_ref as R
from tests import hubert_front_cases as H
from tests import parity as P

pytestmark = pytest.mark.gpu

_STATE = {}
_REF = {}      # N -> (wave, mask, float64 features, e_ref): computed once per length, shared by (a) and (d), never changed
_IDS = {}      # N -> (oracle ids, margins)


def _enc():
    if "enc" not in _STATE:
        from audiotoken_amd.configs import HubertEncoderConfig
        from audiotoken_amd.hubert import HubertEncoder
        _STATE["w"] = H.weights(1)
        _STATE["enc"] = HubertEncoder(HubertEncoderConfig(output_layer=1), device="cuda:0", quantize=True, weights=_STATE["w"])
    return _STATE["enc"], _STATE["w"]


def _ref(N):
    if N not in _REF:
        _, w = _enc()
        wave = H.waveform(N)
        mask = H.ragged_mask(N, wave.shape[0])
        f64 = H.conv_features_f64(w, wave)
        e_ref = (R.conv_features(w, wave).double() - f64).abs().max().item()
        _REF[N] = (wave, mask, f64, e_ref)
    return _REF[N]


def _nan_bytes(n, dev):
    """n bytes of 0xFF: a NaN in every float format the workspace is read as (fp32, float64, fp16 and bf16 pieces)."""
    return torch.full((n,), 0xFF, dtype=torch.uint8, device=dev)


def _features(enc, wave_dev):
    """at_hubert_features over a NaN-filled workspace into a NaN-filled output -> (features on the host, status word)."""
    lib, dev = enc.lib, wave_dev.device
    B, N = wave_dev.shape
    T = lib.at_hubert_num_tokens(N)
    nbytes = lib.at_hubert_workspace_bytes(enc.handle, B, N)
    ws = _nan_bytes(nbytes, dev)
    out = torch.full((B, T, 512), float("nan"), dtype=torch.float32, device=dev)
    status = torch.full((1,), -1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        rc = lib.at_hubert_features(enc.handle, wave_dev.data_ptr(), B, N, out.data_ptr(), ws.data_ptr(), nbytes, _cabi.current_stream_handle(dev),
                                    status.data_ptr())
    _cabi.check(rc, "at_hubert_features")
    torch.cuda.synchronize()
    return out.cpu(), int(status.item())


@pytest.mark.parametrize("arith", list(H.ARITHS))
@pytest.mark.parametrize("N", H.LENGTHS)
def test_features_vs_float64(cuda_device, N, arith):
    enc, _ = _enc()
    wave, _, f64, e_ref = _ref(N)
    enc.set_option("arith", arith)
    try:
        got, status = _features(enc, wave.to(cuda_device))
    finally:
        enc.set_option("arith", "f16x2")
    assert status == 0, f"N={N} {arith}: status {status}"
    assert tuple(got.shape) == tuple(f64.shape)
    assert torch.isfinite(got).all(), f"N={N} {arith}: {int((~torch.isfinite(got)).sum())} features are not finite"
    err = (got.double() - f64).abs()
    worst = np.unravel_index(int(err.argmax()), tuple(err.shape))
    ratio = err.max().item() / e_ref
    print(f"features N={N} L={H.chain(N)[1:]} {arith}: max |got - f64| {err.max().item():.3e} at {worst}, e_ref {e_ref:.3e}, ratio {ratio:.2f} "
          f"(c = {H.C_BAR[arith]:g}), scale {f64.abs().max().item():.2f}")
    assert ratio <= H.C_BAR[arith], f"N={N} {arith}: {err.max().item():.3e} at (clip, frame, channel) {worst} is {ratio:.2f} x e_ref {e_ref:.3e}"


# ---- (b) conv 0 alone ---------------------------------------------------------------------------------------------------------------------------------
def _conv0_wave(kind, N):
    x = H.waveform(N)
    if kind == "dc10":          # DC offset 10, standard deviation 0.01: the variance is 1e-6 of the second moment it is taken from
        x = 10.0 + 0.01 * x
    elif kind == "zero":
        x = torch.zeros_like(x)
    elif kind == "silent_tail":
        x = x.clone()
        x[:, N * 2 // 3:] = 0
    elif kind == "amp1e-4":
        x = 1e-4 * x
    elif kind == "amp1e3":
        x = 1e3 * x
    return x.float().contiguous()


@pytest.mark.parametrize("kind", list(H.C_CONV0))
@pytest.mark.parametrize("N", H.CONV0_N)
def test_conv0_vs_float64(cuda_device, N, kind):
    _, w = _enc()
    lib = _cabi.load()
    w0 = torch.from_numpy(w["feature_extractor.conv_layers.0.conv.weight"])
    g = torch.from_numpy(w["feature_extractor.conv_layers.0.layer_norm.weight"])
    b = torch.from_numpy(w["feature_extractor.conv_layers.0.layer_norm.bias"])
    x = _conv0_wave(kind, N)
    B, T0 = x.shape[0], H.chain(N)[1]
    f64 = H.conv0_f64(x, w0.double(), g.double(), b.double()).transpose(1, 2)
    if kind == "zero":
        f64 = F.gelu(b.double())[None, None, :].expand(B, T0, 512)
    oracle = F.gelu(F.group_norm(F.conv1d(x[:, None], w0, stride=5), 512, g, b, 1e-5)).transpose(1, 2)
    e_ref = (oracle.double() - f64).abs().max().item()
    nbytes = (B * ((T0 + 4095) // 4096) * 520 + 255) // 256 * 256 + B * 4096
    ws = _nan_bytes(nbytes, cuda_device)
    out = torch.full((B, T0, 512), float("nan"), dtype=torch.float32, device=cuda_device)
    dv = [t.contiguous().to(cuda_device) for t in (x, w0.reshape(512, 10), g, b)]
    _cabi.check(lib.at_op_hub_conv0(dv[0].data_ptr(), dv[1].data_ptr(), dv[2].data_ptr(), dv[3].data_ptr(), out.data_ptr(), B, N, ws.data_ptr(), nbytes,
                                    _cabi.current_stream_handle(cuda_device)), "at_op_hub_conv0")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.isfinite(got).all(), f"N={N} {kind}: {int((~torch.isfinite(got)).sum())} outputs are not finite"
    err = (got.double() - f64).abs()
    worst = np.unravel_index(int(err.argmax()), tuple(err.shape))
    ratio = err.max().item() / e_ref
    print(f"conv0 T0={T0} N={N} {kind}: max |got - f64| {err.max().item():.3e} at {worst}, e_ref {e_ref:.3e}, ratio {ratio:.2f} (c = {H.C_CONV0[kind]:g}), "
          f"scale {f64.abs().max().item():.3f}")
    assert ratio <= H.C_CONV0[kind], f"N={N} {kind}: {err.max().item():.3e} at (clip, frame, channel) {worst} is {ratio:.2f} x e_ref {e_ref:.3e}"


# ---- (c) frame mask ------------------------------------------------------------------------------------------------------------------------------------
def _mask_sets(N):
    """Three batches of B = 5 sample masks, or None for the NULL mask. Rows start at every 16-byte alignment when N % 4 != 0."""
    prefix = torch.zeros(5, N)
    for r, s in enumerate((399, 400, 719, 720, N)):
        prefix[r, :min(s, N)] = 1
    other = torch.zeros(5, N)
    other[0, ::2] = 1                          # interior holes: HF uses the sum, not the last valid index
    other[1, N // 3:N // 3 + 400] = 1          # 400 valid samples in the middle of the clip: one frame
    g = torch.Generator().manual_seed(N)
    other[2] = (torch.rand(N, generator=g) < 0.7).float()
    other[3, :N - 1] = 1
    # row 4: all zero -> no valid frame
    return {"prefix": prefix, "holes": other, "null": None}


@pytest.mark.parametrize("which", ["prefix", "holes", "null"])
@pytest.mark.parametrize("N", [401, 4099, 16384, 16385, 16386, 16387, 65541])
def test_frame_mask_is_exact(cuda_device, N, which):
    lib = _cabi.load()
    B, T = 5, H.chain(N)[7]
    mask = _mask_sets(N)[which]
    want = torch.ones(B, T) if mask is None else R.frame_mask(mask, T).float()
    if which == "prefix":
        assert want.sum(-1).tolist() == [max(0, min(H.frame_len(min(s, N)), T)) for s in (399, 400, 719, 720, N)]
    out = torch.full((B, T), float("nan"), dtype=torch.float32, device=cuda_device)
    m = None if mask is None else mask.to(cuda_device)
    _cabi.check(lib.at_op_hub_frame_mask(_cabi.ptr(m), out.data_ptr(), B, N, T, _cabi.current_stream_handle(cuda_device)), "at_op_hub_frame_mask")
    torch.cuda.synchronize()
    got = out.cpu()
    assert torch.equal(got, want), f"N={N} {which}: valid frames per clip {got.sum(-1).tolist()}, oracle {want.sum(-1).tolist()}"


# ---- (d) ids end to end --------------------------------------------------------------------------------------------------------------------------------
def _oracle_ids(N):
    if N not in _IDS:
        _, w = _enc()
        wave, mask, _, _ = _ref(N)
        _IDS[N] = R.semantic_s_encode(w, wave, mask, 1, return_margins=True)
    return _IDS[N]


@pytest.mark.parametrize("arith", list(H.ARITHS))
@pytest.mark.parametrize("N", H.IDS_LENGTHS)
def test_ids_vs_oracle(cuda_device, N, arith):
    enc, _ = _enc()
    wave, mask, _, _ = _ref(N)
    ref, margins = _oracle_ids(N)
    enc.set_option("arith", arith)
    try:
        toks = enc(wave.to(cuda_device), mask.to(cuda_device))
        status = enc.last_status()
    finally:
        enc.set_option("arith", "f16x2")
    assert status == 0 and toks.shape == ref.shape
    P.assert_tokens_equal_or_explained(toks, ref, margins, P.VQ_TIE, f"semantic_s one layer N={N} {arith}")


@pytest.mark.parametrize("arith", list(H.ARITHS))
def test_a_clip_without_a_valid_frame_leaves_the_others_alone(cuda_device, arith):
    """Mask sum 399 on the middle clip of a batch: no valid frame. HF's own result for that clip is a softmax over all-masked keys and is not pinned here —
    its outputs must be finite; the other clips still match the oracle."""
    enc, w = _enc()
    N = 720
    wave = H.waveform(N, 3)
    mask = torch.ones(3, N)
    mask[1, 399:] = 0
    ref, margins = R.semantic_s_encode(w, wave, mask, 1, return_margins=True)
    enc.set_option("arith", arith)
    try:
        toks, hid = enc(wave.to(cuda_device), mask.to(cuda_device), return_hidden=True)
        status = enc.last_status()
    finally:
        enc.set_option("arith", "f16x2")
    assert status == 0
    assert torch.isfinite(hid).all(), f"{arith}: hidden state has {int((~torch.isfinite(hid)).sum())} non-finite values"
    assert int(toks.min()) >= 0 and int(toks.max()) < 1000
    keep = [0, 2]
    P.assert_tokens_equal_or_explained(toks.cpu()[keep], ref[keep], margins[keep], P.VQ_TIE, f"clips beside one without a valid frame, {arith}")


# ---- (e) positional conv -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", list(H.POSCONV_T))
def test_positional_conv_at_tile_and_halo_seams(cuda_device, T):
    """Hidden state 0 (n_layers = 0) with the LDS-resident split kernel (posconv_split = 1) and with the 16 fp32 windowed GEMMs (= 0): each within 1e-4 of
    the oracle's states[0]; ids of the one-layer model identical between the two."""
    enc, w = _enc()
    N = H.POSCONV_T[T]
    wave, mask, _, _ = _ref(N)
    want = R.hidden_states(w, wave, mask, 0, return_all=True)[0]
    assert want.shape[1] == T
    x, m = wave.to(cuda_device), mask.to(cuda_device)
    seen = {}
    try:
        for setting in (1, 0):
            enc.set_option("posconv_split", setting)
            _, hid = enc(x, m, n_layers=0, return_hidden=True)
            ids = enc(x, m)
            assert enc.last_status() == 0
            seen[setting] = ((hid.cpu() - want).abs().max().item(), ids.cpu())
    finally:
        enc.set_option("posconv_split", 1)
    print(f"positional conv T={T} N={N}: max |hidden state 0 - oracle| split kernel {seen[1][0]:.2e}, fp32 GEMMs {seen[0][0]:.2e} "
          f"(max |h| {want.abs().max().item():.2f})")
    assert seen[1][0] <= 1e-4 and seen[0][0] <= 1e-4
    assert torch.equal(seen[1][1], seen[0][1])
