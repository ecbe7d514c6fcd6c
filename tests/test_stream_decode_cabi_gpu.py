"""GPU: at_encodec_decode_stream_* through ctypes — the transaction rule, independent streams on one handle, and every argument error
(an error return with at_last_error set; nothing is launched and the device stays usable)."""
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import weights as W
from audiotoken_amd.streaming import HOP
from oracle import encodec_ref as R

pytestmark = pytest.mark.gpu

K = 8


@pytest.fixture(scope="module")
def dec_weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True, family="trained_like")


@pytest.fixture(scope="module")
def decoder(cuda_device, dec_weights):
    from audiotoken_amd.configs import AcousticDecoderConfig
    from audiotoken_amd.decoder import AcousticDecoder
    return AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=dec_weights)


class Raw:
    """The four entry points on one handle; every state buffer is a uint8 device tensor the caller keeps."""

    def __init__(self, dec):
        self.dec, self.lib, self.h = dec, dec._h.lib, dec._h.handle
        self.stream = _cabi.current_stream_handle(dec.device)

    def state(self, B, reset=True):
        s = torch.empty(self.lib.at_encodec_decode_stream_state_bytes(self.h, B), dtype=torch.uint8, device=self.dec.device)
        if reset:
            assert self.lib.at_encodec_decode_stream_reset(self.h, s.data_ptr(), B, self.stream) == 0, _cabi.last_error()
        return s

    def push(self, s_in, s_out, codes, ws_bytes=None, B=None):
        codes = codes.contiguous()   # the library reads [B][K][t] densely
        Bc, Kc, t = codes.shape
        B = Bc if B is None else B
        wav = torch.zeros((Bc, HOP * max(t, 1)), dtype=torch.float32, device=self.dec.device)
        need = self.lib.at_encodec_decode_stream_workspace_bytes(self.h, max(B, 1), max(t, 1))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=self.dec.device)
        status = torch.zeros(1, dtype=torch.int32, device=self.dec.device)
        rc = self.lib.at_encodec_decode_stream_checked(self.h, _cabi.ptr(s_in), _cabi.ptr(s_out), codes.data_ptr(), B, Kc, t, wav.data_ptr(), ws.data_ptr(),
                                                       need if ws_bytes is None else ws_bytes, self.stream, status.data_ptr())
        return rc, wav, (int(status.item()) if rc == 0 else None)


def _codes(B, T, seed):
    return torch.randint(0, 1024, (B, K, T), dtype=torch.long, generator=torch.Generator().manual_seed(seed)).cuda()


def test_state_size_and_workspace(decoder):
    raw = Raw(decoder)
    assert raw.lib.at_encodec_decode_stream_state_bytes(raw.h, 1) == 4 * (6 * 128 + 4 * 512 + 2 * 512)
    assert raw.lib.at_encodec_decode_stream_state_bytes(raw.h, 5) == 5 * raw.lib.at_encodec_decode_stream_state_bytes(raw.h, 1)
    assert raw.lib.at_encodec_decode_stream_state_bytes(raw.h, 0) == 0
    assert raw.lib.at_encodec_decode_stream_workspace_bytes(raw.h, 1, 0) == 0
    # a push's workspace does not depend on what was pushed before and stays near the one-shot workspace of its window
    assert raw.lib.at_encodec_decode_stream_workspace_bytes(raw.h, 2, 75) < raw.lib.at_encodec_decode_workspace_bytes(raw.h, 2, 80)


def test_repeated_push_from_the_same_state_is_identical(decoder):
    """Transaction: state_in is only read, so the same push from the same state_in gives the same audio and the same state_out."""
    raw = Raw(decoder)
    B = 2
    s0, s1, s2, s3 = raw.state(B), raw.state(B, reset=False), raw.state(B, reset=False), raw.state(B, reset=False)
    codes = _codes(B, 30, 1)
    rc, first, status = raw.push(s0, s1, codes[:, :, :12])
    assert rc == 0 and status == 0, _cabi.last_error()
    s1_copy = s1.clone()
    new = codes[:, :, 12:17]
    rc, a, status = raw.push(s1, s2, new)
    assert rc == 0 and status == 0, _cabi.last_error()
    rc, b, status = raw.push(s1, s3, new)
    assert rc == 0 and status == 0, _cabi.last_error()
    assert torch.equal(a, b) and torch.equal(s2, s3)
    assert torch.equal(s1, s1_copy), "a push must not write state_in"
    assert not torch.equal(s2, s1)
    # and the stream goes on from either copy
    rc, c, _ = raw.push(s2, s1, codes[:, :, 17:])
    assert rc == 0, _cabi.last_error()
    ref = R.acoustic_decode(W.synth_encodec_weights(seed=0, with_decoder=True, family="trained_like"), codes.cpu()).reshape(B, -1)
    got = torch.cat([first, a, c], dim=1).cpu()
    assert (got - ref).abs().max().item() < 1e-3


def test_two_interleaved_streams_do_not_disturb_each_other(decoder):
    raw = Raw(decoder)
    ca, cb = _codes(1, 40, 2), _codes(3, 33, 3)
    sched_a, sched_b = [7, 1, 1, 10, 21], [9, 2, 1, 21]

    def alone(codes, sched):
        B = codes.shape[0]
        s = [raw.state(B), raw.state(B, reset=False)]
        out, pos = [], 0
        for n in sched:
            rc, w, status = raw.push(s[0], s[1], codes[:, :, pos:pos + n])
            assert rc == 0 and status == 0, _cabi.last_error()
            out.append(w)
            s.reverse()
            pos += n
        return torch.cat(out, dim=1)

    ref_a, ref_b = alone(ca, sched_a), alone(cb, sched_b)
    sa, sb = [raw.state(1), raw.state(1, reset=False)], [raw.state(3), raw.state(3, reset=False)]
    out_a, out_b, pa, pb = [], [], 0, 0
    for i in range(max(len(sched_a), len(sched_b))):
        if i < len(sched_a):
            rc, w, status = raw.push(sa[0], sa[1], ca[:, :, pa:pa + sched_a[i]])
            assert rc == 0 and status == 0, _cabi.last_error()
            out_a.append(w); sa.reverse(); pa += sched_a[i]
        if i < len(sched_b):
            rc, w, status = raw.push(sb[0], sb[1], cb[:, :, pb:pb + sched_b[i]])
            assert rc == 0 and status == 0, _cabi.last_error()
            out_b.append(w); sb.reverse(); pb += sched_b[i]
    assert torch.equal(torch.cat(out_a, dim=1), ref_a) and torch.equal(torch.cat(out_b, dim=1), ref_b)


def _refused(rc, needle):
    assert rc != 0
    msg = _cabi.last_error()
    assert needle in msg, msg


def test_argument_errors_return_and_leave_the_device_usable(cuda_device, dec_weights):
    # a handle of its own: the library's note per state ADDRESS would otherwise know addresses the allocator reuses from the tests above
    from audiotoken_amd.configs import AcousticDecoderConfig
    from audiotoken_amd.decoder import AcousticDecoder
    raw = Raw(AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=dec_weights))
    B = 2
    s0, s1 = raw.state(B), raw.state(B, reset=False)
    codes = _codes(B, 20, 4)
    _refused(raw.push(None, s1, codes)[0], "null state")
    _refused(raw.push(s0, None, codes)[0], "null state")
    _refused(raw.push(s0, s0, codes)[0], "two buffers")
    _refused(raw.push(s1, s0, codes)[0], "neither reset")                      # an un-reset state
    _refused(raw.push(s0, s1, _codes(3, 20, 4))[0], "another B")               # a state for another B
    _refused(raw.push(s0, s1, codes[:, :, :0])[0], "t_new >= 1")               # t_new < 1
    _refused(raw.push(s0, s1, codes[:, :, :6])[0], "at least 7 frames")        # a first push below 7 frames
    _refused(raw.push(s0, s1, codes, ws_bytes=1024)[0], "workspace too small")
    # an encode stream's state is refused by the decode push, a decode state by the encode push
    lib, h = raw.lib, raw.h
    e0 = torch.empty(lib.at_encodec_stream_state_bytes(h, B), dtype=torch.uint8, device="cuda:0")
    e1 = torch.empty_like(e0)
    assert lib.at_encodec_stream_reset(h, e0.data_ptr(), B, raw.stream) == 0
    _refused(raw.push(e0, s1, codes)[0], "encode stream")
    wav = torch.zeros(B, 7 * HOP, device="cuda:0")
    out_codes = torch.zeros((B, K, 7), dtype=torch.int16, device="cuda:0")
    ws = torch.empty(lib.at_encodec_stream_workspace_bytes(h, B, 7 * HOP), dtype=torch.uint8, device="cuda:0")
    import ctypes as C
    t_out = C.c_int(0)
    big = torch.empty(max(e0.numel(), s0.numel()), dtype=torch.uint8, device="cuda:0")
    rc = lib.at_encodec_encode_stream_checked(h, s0.data_ptr(), big.data_ptr(), wav.data_ptr(), B, 7 * HOP, 0, K, out_codes.data_ptr(), C.byref(t_out), None,
                                              ws.data_ptr(), ws.numel(), raw.stream, None)
    _refused(rc, "decode stream")
    del e1
    # the stream is still usable after all of that
    rc, w, status = raw.push(s0, s1, codes)
    assert rc == 0 and status == 0, _cabi.last_error()
    ref = R.acoustic_decode(dec_weights, codes.cpu()).reshape(B, -1)
    assert (w.cpu() - ref).abs().max().item() < 1e-3


def test_handle_without_decoder_is_refused(cuda_device):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    enc = AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=W.synth_encodec_weights(seed=0, with_decoder=False))
    lib, h = enc._h.lib, enc._h.handle
    s = torch.empty(lib.at_encodec_decode_stream_state_bytes(h, 1), dtype=torch.uint8, device="cuda:0")
    s2 = torch.empty_like(s)
    _refused(lib.at_encodec_decode_stream_reset(h, s.data_ptr(), 1, _cabi.current_stream_handle(enc.device)), "decoder")
    codes = _codes(1, 8, 5)
    wav = torch.zeros(1, 8 * HOP, device="cuda:0")
    ws = torch.empty(1 << 20, dtype=torch.uint8, device="cuda:0")
    rc = lib.at_encodec_decode_stream_checked(h, s.data_ptr(), s2.data_ptr(), codes.data_ptr(), 1, K, 8, wav.data_ptr(), ws.data_ptr(), ws.numel(),
                                              _cabi.current_stream_handle(enc.device), None)
    _refused(rc, "decoder")
