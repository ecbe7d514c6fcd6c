"""GPU: the error contract of the streaming entry points (include/audiotoken_hip.h): every argument error returns non-zero with a message in
at_last_error(), nothing is launched, and the device stays usable — the next valid push succeeds."""
import ctypes as C

import pytest
import torch

from audiotoken_amd import _cabi, weights as W

pytestmark = pytest.mark.gpu


def test_stream_argument_validation(cuda_device):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    lib, h = enc._h.lib, enc._h.handle
    B, n = 2, 3200
    stream = _cabi.current_stream_handle(torch.device("cuda:0"))
    sbytes = lib.at_encodec_stream_state_bytes(h, B)
    assert sbytes == B * (640 + 4 * 512 + 6 * 512) * 4 and lib.at_encodec_stream_state_bytes(h, 0) == 0
    s0 = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    s1 = torch.empty(sbytes, dtype=torch.uint8, device="cuda")
    wav = torch.from_numpy(W.synth_waveform(B, 2 * n, 24000, seed=3)).cuda()
    codes = torch.zeros(B, 8, 10, dtype=torch.int16, device="cuda")
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = lib.at_encodec_stream_workspace_bytes(h, B, n)
    assert nbytes > 0 and lib.at_encodec_stream_workspace_bytes(h, 0, n) == 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    t_out = C.c_int(-1)

    def push(sin, sout, x, n_new, final, wbytes=nbytes, nq=8):
        return lib.at_encodec_encode_stream_checked(h, sin, sout, x.data_ptr(), B, n_new, final, nq, codes.data_ptr(), C.byref(t_out), None,
                                                    ws.data_ptr(), wbytes, stream, status.data_ptr())

    # a state the handle has never seen
    assert push(s0.data_ptr(), s1.data_ptr(), wav, n, 0) != 0 and "reset" in _cabi.last_error()
    assert lib.at_encodec_stream_reset(h, None, B, stream) != 0 and _cabi.last_error()
    assert lib.at_encodec_stream_reset(h, s0.data_ptr(), B, stream) == 0
    # null state, one buffer for both, n_new not a multiple of 320, first push too short, workspace too small, another B, too many codebooks
    assert push(None, s1.data_ptr(), wav, n, 0) != 0 and "null state" in _cabi.last_error()
    assert push(s0.data_ptr(), None, wav, n, 0) != 0 and "null state" in _cabi.last_error()
    assert push(s0.data_ptr(), s0.data_ptr(), wav, n, 0) != 0 and "two buffers" in _cabi.last_error()
    assert push(s0.data_ptr(), s1.data_ptr(), wav, n - 1, 0) != 0 and "320" in _cabi.last_error()
    assert push(s0.data_ptr(), s1.data_ptr(), wav, 0, 0) != 0 and "320" in _cabi.last_error()
    assert push(s0.data_ptr(), s1.data_ptr(), wav, 640, 0) != 0 and "first push" in _cabi.last_error()
    assert push(s0.data_ptr(), s1.data_ptr(), wav, n, 0, wbytes=nbytes // 2) != 0 and "workspace" in _cabi.last_error()
    assert push(s0.data_ptr(), s1.data_ptr(), wav, n, 0, nq=64) != 0 and _cabi.last_error()
    assert lib.at_encodec_encode_stream_checked(h, s0.data_ptr(), s1.data_ptr(), wav.data_ptr(), B + 1, n, 0, 8, codes.data_ptr(), None, None,
                                                ws.data_ptr(), nbytes, stream, status.data_ptr()) != 0 and "another B" in _cabi.last_error()
    # the device stays usable: a valid first push, a valid second push behind it (n_new = 320 is fine once the stream has started)
    assert push(s0.data_ptr(), s1.data_ptr(), wav, n, 0) == 0 and t_out.value == 10
    assert int(status.item()) == 0
    first = codes.clone()
    assert push(s1.data_ptr(), s0.data_ptr(), wav[:, n:].contiguous(), 320, 0) == 0 and t_out.value == 1
    # the final push, then a push after it
    tail = wav[:, n + 320:n + 320 + 333].contiguous()
    assert push(s0.data_ptr(), s1.data_ptr(), tail, 333, 1) == 0 and t_out.value == 2
    assert int(status.item()) == 0
    assert push(s1.data_ptr(), s0.data_ptr(), wav, n, 0) != 0 and "after the final push" in _cabi.last_error()
    # a failed call changed nothing: reset and the first push gives the first push's codes again
    assert lib.at_encodec_stream_reset(h, s1.data_ptr(), B, stream) == 0
    assert push(s1.data_ptr(), s0.data_ptr(), wav, n, 0) == 0
    assert torch.equal(codes, first)
    # a final push without samples ends a frame-aligned stream with T = 0
    assert push(s0.data_ptr(), s1.data_ptr(), wav, 0, 1) == 0 and t_out.value == 0
    torch.cuda.synchronize()
