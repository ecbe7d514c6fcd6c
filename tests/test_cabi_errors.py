"""The C ABI's error contract (include/audiotoken_hip.h): every entry point returns an error code and leaves a message in
at_last_error(); nothing aborts, nothing falls back. CPU part: the pure helper functions and the no-GPU failures; GPU
part: argument validation of the encode / decode / operator calls."""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi, weights as W
from tests import parity as P


def test_token_count_helpers_match_the_reference_formulas():
    lib = _cabi.load()
    from oracle import hubert_ref, w2vbert_ref
    for n in (400, 16000, 47999, 480000):
        assert lib.at_hubert_num_tokens(n) == hubert_ref.num_frames(n)
    for n, pad in ((16000, 2), (480000, 2), (12345, 2), (16000, 1)):
        feats, _ = w2vbert_ref.processor(torch.zeros(1, n), torch.ones(1, n), pad)
        assert lib.at_w2vbert_num_tokens(n, pad) == feats.shape[1]


def test_null_handles_are_rejected_with_a_message():
    lib = _cabi.load()
    assert lib.at_encodec_finalize(None, 0) != 0 and _cabi.last_error()
    assert lib.at_w2vbert_finalize(None) != 0 and _cabi.last_error()
    assert lib.at_hubert_finalize(None) != 0 and _cabi.last_error()
    assert lib.at_op_gemm(None, None) != 0 and "null" in _cabi.last_error().lower()
    assert lib.at_encodec_workspace_bytes(None, 0, 0) == 0


def test_gemm_dual_second_source_width_must_be_a_multiple_of_4():
    """The general body fetches 16-byte chunks: a second source of 6 columns would have its last chunk read past the X2 row and the weight row.
    The argument check refuses the call before anything is launched (status -1, message set), so this runs without a device; the addresses
    are never dereferenced."""
    lib = _cabi.load()
    d = _cabi.GemmDesc()
    d.X, d.x_bstride, d.Tin, d.Cin, d.ldx = 4096, 0, 64, 16, 16
    d.ktaps, d.stride, d.pad_left, d.pad_mode = 1, 1, 0, 0
    d.W, d.bias, d.C, d.c_bstride, d.ldc = 8192, 0, 12288, 0, 32
    d.R, d.r_bstride, d.ldr = 0, 0, 32
    d.M, d.N, d.K, d.batch, d.pro, d.epi, d.alpha = 64, 32, 16 + 6, 1, 0, 0, 1.0
    assert lib.at_op_gemm_dual(C.byref(d), 16384, 0, 8, 16, None) == -1
    assert "width of the second source must be a multiple of 4" in _cabi.last_error()
    assert lib.at_op_gemm_dual(C.byref(d), None, 0, 8, 16, None) == -1 and "second source" in _cabi.last_error()
    assert lib.at_op_gemm_dual(None, 16384, 0, 8, 16, None) == -1 and "null" in _cabi.last_error().lower()
    assert lib.at_op_attention_f32(None, None, None, None, 1, 1, 16, None) == -1 and "bad arguments" in _cabi.last_error()
    assert lib.at_op_attention_f32(4096, 4096, None, 4096, 1, 1, 65, None) == -1 and "bad arguments" in _cabi.last_error()


def test_hubert_front_taps_refuse_bad_arguments_before_any_launch():
    """at_hubert_features, at_op_hub_conv0 and at_op_hub_frame_mask: every refusal below happens in the argument checks (status -1, message set), so this
    runs without a device; the addresses are never dereferenced."""
    lib = _cabi.load()
    assert lib.at_hubert_features(None, 4096, 1, 400, 4096, 4096, 1 << 30, None, None) == -1 and "not finalized" in _cabi.last_error()
    ok = dict(wav=4096, w=8192, gamma=12288, beta=16384, out=20480, B=2, N=403, ws=1 << 20, nbytes=1280 + 2 * 4096)

    def conv0(**kw):
        a = dict(ok, **kw)
        return lib.at_op_hub_conv0(a["wav"], a["w"], a["gamma"], a["beta"], a["out"], a["B"], a["N"], a["ws"], a["nbytes"], None)

    for name in ("wav", "w", "gamma", "beta", "out", "ws"):
        assert conv0(**{name: None}) == -1 and "null pointer" in _cabi.last_error(), name
    assert conv0(N=9) == -1 and "N >= 10" in _cabi.last_error()
    assert conv0(B=0) == -1 and "B >= 1" in _cabi.last_error()
    assert conv0(ws=(1 << 20) + 8) == -1 and "16-byte aligned" in _cabi.last_error()
    # T0 = 79: one chunk of 65 doubles per clip = 1040 bytes -> 1280, + 2 x 4096 for scale / shift; one byte less is refused
    assert conv0(nbytes=1280 + 8192 - 1) == -1 and "workspace too small" in _cabi.last_error()
    # T0 = 4097 takes a second chunk of moment partials: what was enough for T0 = 4096 no longer is
    enough_4096 = (2 * 1 * 520 + 255) // 256 * 256 + 8192
    assert conv0(N=5 * 4097 + 5, nbytes=enough_4096) == -1 and "workspace too small" in _cabi.last_error()
    assert lib.at_op_hub_frame_mask(4096, None, 2, 400, 1, None) == -1 and "null pointer" in _cabi.last_error()
    for B, N, T in ((0, 400, 1), (2, 0, 1), (2, 400, 0)):
        assert lib.at_op_hub_frame_mask(4096, 8192, B, N, T, None) == -1 and "B, N, T >= 1" in _cabi.last_error()


@pytest.mark.gpu
def test_hubert_features_argument_validation(cuda_device):
    """at_hubert_features on a finalized handle: null pointers, a clip below 400 samples and a short workspace are refused with a message, nothing is
    written, and the handle serves the next call."""
    from audiotoken_amd.configs import HubertEncoderConfig
    from audiotoken_amd.hubert import HubertEncoder
    enc = HubertEncoder(HubertEncoderConfig(output_layer=0), device="cuda:0", quantize=False, weights=W.synth_hubert_weights(0, 2, False))
    lib, h = enc.lib, enc.handle
    B, N = 2, 405
    wav = torch.zeros(B, N, device="cuda")
    feats = torch.full((B, 1, 512), float("nan"), device="cuda")
    nbytes = lib.at_hubert_workspace_bytes(h, B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _cabi.current_stream_handle(torch.device("cuda:0"))
    assert lib.at_hubert_features(h, None, B, N, feats.data_ptr(), ws.data_ptr(), nbytes, st, None) == -1 and "null pointer" in _cabi.last_error()
    assert lib.at_hubert_features(h, wav.data_ptr(), B, N, None, ws.data_ptr(), nbytes, st, None) == -1 and "null pointer" in _cabi.last_error()
    assert lib.at_hubert_features(h, wav.data_ptr(), B, N, feats.data_ptr(), None, nbytes, st, None) == -1 and "null pointer" in _cabi.last_error()
    assert lib.at_hubert_features(h, wav.data_ptr(), B, 399, feats.data_ptr(), ws.data_ptr(), nbytes, st, None) == -1 and "too short" in _cabi.last_error()
    assert lib.at_hubert_features(h, wav.data_ptr(), 0, N, feats.data_ptr(), ws.data_ptr(), nbytes, st, None) == -1 and "too short" in _cabi.last_error()
    assert lib.at_hubert_features(h, wav.data_ptr(), B, N, feats.data_ptr(), ws.data_ptr(), nbytes - 1, st, None) == -1 and "workspace" in _cabi.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(feats).all()), "a refused call must not write features"
    assert lib.at_hubert_features(h, wav.data_ptr(), B, N, feats.data_ptr(), ws.data_ptr(), nbytes, st, None) == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(feats).all())


@pytest.mark.gpu
def test_encode_argument_validation(cuda_device):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    lib, h = enc._h.lib, enc._h.handle
    B, N = 2, 3200
    wav = torch.zeros(B, N, device="cuda")
    codes = torch.zeros(B, 8, 10, dtype=torch.int16, device="cuda")
    nbytes = lib.at_encodec_workspace_bytes(h, B, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _cabi.current_stream_handle(torch.device("cuda:0"))
    ok = lib.at_encodec_encode(h, wav.data_ptr(), None, B, N, 8, codes.data_ptr(), None, None, ws.data_ptr(), nbytes, st)
    assert ok == 0
    # workspace too small, too many codebooks, null output: error code + message, the handle stays usable
    assert lib.at_encodec_encode(h, wav.data_ptr(), None, B, N, 8, codes.data_ptr(), None, None, ws.data_ptr(), nbytes // 2, st) != 0
    assert "workspace" in _cabi.last_error()
    assert lib.at_encodec_encode(h, wav.data_ptr(), None, B, N, 64, codes.data_ptr(), None, None, ws.data_ptr(), nbytes, st) != 0
    assert _cabi.last_error()
    assert lib.at_encodec_encode(h, wav.data_ptr(), None, B, N, 8, None, None, None, ws.data_ptr(), nbytes, st) != 0
    assert lib.at_encodec_set_option(h, b"no_such_option", 1) != 0
    # decode on a handle finalized without the decoder
    assert lib.at_encodec_decode(h, codes.data_ptr(), B, 8, 10, wav.data_ptr(), ws.data_ptr(), nbytes, st) != 0
    assert "decoder" in _cabi.last_error()
    assert lib.at_encodec_encode(h, wav.data_ptr(), None, B, N, 8, codes.data_ptr(), None, None, ws.data_ptr(), nbytes, st) == 0
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_clip_below_the_minimum_length_is_refused(cuda_device):
    """N = 320 (L[3] = 8: the stage-3 strided conv would reflect all of its input) returns an error with a message; nothing is written,
    and the handle encodes the shortest valid clip (N = 321, T = 2) to the oracle's ids right afterwards."""
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    from oracle import encodec_ref as R
    w = W.synth_encodec_weights(seed=0, with_decoder=False)
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=w)
    lib, h = enc._h.lib, enc._h.handle
    B = 2
    wav = torch.from_numpy(W.synth_waveform(B, 321, 24000, seed=7321)).cuda()
    codes = torch.full((B, 8, 2), -1, dtype=torch.int16, device="cuda")
    nbytes = lib.at_encodec_workspace_bytes(h, B, 321)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    st = _cabi.current_stream_handle(torch.device("cuda:0"))
    short = wav[:, :320].contiguous()
    for n, message in ((320, "too short for the strided convs"), (9, "N >= 10")):
        assert lib.at_encodec_encode(h, short.data_ptr(), None, B, n, 8, codes.data_ptr(), None, None, ws.data_ptr(), nbytes, st) != 0
        assert message in _cabi.last_error(), (n, _cabi.last_error())
    torch.cuda.synchronize()
    assert bool((codes == -1).all()), "a refused call must not write codes"
    with pytest.raises(_cabi.HipLibraryError, match="too short"):
        enc(short)
    t_out = C.c_int(0)
    assert lib.at_encodec_encode(h, wav.data_ptr(), None, B, 321, 8, codes.data_ptr(), C.byref(t_out), None, ws.data_ptr(), nbytes, st) == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert t_out.value == 2
    ref, margins = R.acoustic_encode(w, wav.cpu(), 8, return_margins=True)
    P.assert_rvq_equal_or_explained(codes.cpu(), ref, margins, P.RVQ_TIE, "N=321 after a refused call")


@pytest.mark.gpu
def test_finalize_reports_missing_tensors(cuda_device):
    lib = _cabi.load()
    h = lib.at_encodec_create(0)
    assert h
    try:
        arr = np.zeros((32, 1, 7), dtype=np.float32)
        _cabi.set_tensor(lib, lib.at_encodec_set_tensor, h, "encoder.model.0.conv.conv.weight", arr)
        assert lib.at_encodec_finalize(h, 0) != 0
        assert _cabi.last_error()
    finally:
        lib.at_encodec_destroy(h)


@pytest.mark.gpu
def test_gemm_descriptor_validation(cuda_device):
    lib = _cabi.load()
    x = torch.zeros(64, 30, device="cuda")
    d = _cabi.GemmDesc()
    d.X, d.x_bstride, d.Tin, d.Cin, d.ldx = x.data_ptr(), 0, 64, 30, 30        # Cin not a multiple of 4
    d.ktaps, d.stride, d.pad_left, d.pad_mode = 1, 1, 0, 0
    d.W, d.bias, d.C, d.c_bstride, d.ldc = x.data_ptr(), 0, x.data_ptr(), 0, 32
    d.R, d.r_bstride, d.ldr = 0, 0, 32
    d.M, d.N, d.K, d.batch, d.pro, d.epi, d.alpha = 64, 32, 30, 1, 0, 0, 1.0
    assert lib.at_op_gemm(C.byref(d), _cabi.current_stream_handle(torch.device("cuda:0"))) != 0
    assert "multiple" in _cabi.last_error()
