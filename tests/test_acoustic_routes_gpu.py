"""GPU: the acoustic encoder against the CPU oracle on EVERY length-selected kernel route (tests/acoustic_routes.py: 32 signatures at their
smallest length, 16 mid lengths with ragged last tiles, the 256-row seams of the padded GEMM operands), on both weight families, with the
route that ran read back from the handle's profile groups and range report — plus the batch-side cross (B = 81, subbatch 2), the short
clips through AudioToken.encode, the unchecked C entry point and AcousticStream.flush.

Every case prints one `route-matrix` line; profiles/acoustic_route_matrix.txt holds those lines of one run (`pytest -s` shows them)."""
import ctypes as C

import pytest
import torch

from audiotoken_amd import _cabi, weights as W
from oracle import encodec_ref as R
from tests import acoustic_routes as AR
from tests import parity as P

pytestmark = pytest.mark.gpu

EMB_TOL = 1e-3     # the project's contract for float intermediates (README, test_encode_matches_golden)


@pytest.fixture(scope="module")
def families(cuda_device):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    out = {}
    for family in AR.FAMILIES:
        w = W.synth_encodec_weights(seed=0, with_decoder=False, family=family)
        out[family] = (w, AcousticEncoder(AcousticEncoderConfig(bandwidth=6), device="cuda:0", weights=w))
    return out


def _encode_with_evidence(enc, wav):
    """One encode with the profile taps on: (codes, emb, {group: launches}, range report)."""
    enc.enable_profile(True)
    try:
        codes, emb = enc(wav.cuda(), None, return_embeddings=True)
        assert enc.last_status() == 0, f"status word {enc.last_status()}"
        launches = {k: v[1] for k, v in enc.read_profile().items()}
    finally:
        enc.enable_profile(False)
    return codes.cpu(), emb.cpu(), launches, enc.range_report()


def _check_route(sig, launches, sites, n_sub=1):
    """The profile groups / launch counts and the range sites must be the ones the signature predicts (the conv stack runs once per sub-batch)."""
    for group, per_sub in AR.expected_launches(sig).items():
        want = per_sub * (1 if group == "final_conv" else n_sub)
        assert launches.get(group, 0) == want, f"signature {sig}: profile group {group} has {launches.get(group, 0)} launches, the route predicts {want} ({launches})"
    for site, ran in AR.expected_range_sites(sig).items():
        assert (sites[site] > 0.0) == ran, f"signature {sig}: range site {site} reads {sites[site]}, the route predicts {'> 0' if ran else '0.0'}"


def _check_against_oracle(w, wav, codes, emb, what):
    """Embeddings within 1e-3, ids equal or explained — and equal outright wherever the oracle's margins allow no explanation.
    Returns (embedding error, embedding scale, differing ids, the oracle's smallest margin)."""
    emb_ref = R.seanet_encode(w, wav).permute(0, 2, 1)
    ref, margins = R.acoustic_encode(w, wav, AR.N_Q, return_margins=True)
    assert tuple(codes.shape) == tuple(ref.shape) and codes.dtype == torch.int16
    err, scale = (emb - emb_ref).abs().max().item(), emb_ref.abs().max().item()
    min_margin = float(margins.min())
    print(f"{what}: emb max abs err {err:.3e} (|emb| max {scale:.2f}), oracle min margin {min_margin:.2e}")
    assert err < EMB_TOL, f"{what}: embedding differs from the oracle by {err:.3e}"
    n_ids = P.assert_rvq_equal_or_explained(codes, ref, margins, P.RVQ_TIE, what)
    if min_margin >= P.RVQ_TIE:
        assert torch.equal(codes, ref), f"{what}: ids differ although no oracle margin is below {P.RVQ_TIE:g}"
    return err, scale, n_ids, min_margin


@pytest.mark.parametrize("family", AR.FAMILIES)
@pytest.mark.parametrize("N", AR.LENGTHS)
def test_route_matches_oracle(N, family, families):
    w, enc = families[family]
    sig = AR.signature(N)
    wav = torch.from_numpy(AR.waveform(N))
    codes, emb, launches, sites = _encode_with_evidence(enc, wav)
    _check_route(sig, launches, sites)
    err, scale, n_ids, min_margin = _check_against_oracle(w, wav, codes, emb, f"N={N} {family} {sig}")
    print(f"route-matrix N={N} family={family} sig={''.join(map(str, sig))} L={AR.chain(N)[1:]} emb_err={err:.3e} emb_scale={scale:.2f} "
          f"ids_differ={n_ids} oracle_min_margin={min_margin:.2e}")


@pytest.mark.parametrize("N", AR.BATCH_CROSS)
def test_batch_cross_matches_oracle(N, families):
    """B = 81 (one past the pipelined LSTM's limit) in sub-batches of 2 (41 conv-stack passes, the last of one clip): launch_copy_rows, the sub-batch
    tail and the LSTM route choice at ragged lengths."""
    w, enc = families["uniform"]
    Bc, sub = AR.BATCH_CROSS_B, AR.BATCH_CROSS_SUBBATCH
    sig = AR.signature(N)
    wav = torch.from_numpy(AR.waveform(N, Bc))
    before = enc.get_option("subbatch")
    enc.set_option("subbatch", sub)
    try:
        codes, emb, launches, sites = _encode_with_evidence(enc, wav)
    finally:
        enc.set_option("subbatch", before)
    assert enc.get_option("subbatch") == before
    _check_route(sig, launches, sites, n_sub=-(-Bc // sub))
    err, scale, n_ids, min_margin = _check_against_oracle(w, wav, codes, emb, f"N={N} B={Bc} subbatch={sub} {sig}")
    print(f"route-matrix N={N} family=uniform sig={''.join(map(str, sig))} B={Bc} subbatch={sub} emb_err={err:.3e} emb_scale={scale:.2f} "
          f"ids_differ={n_ids} oracle_min_margin={min_margin:.2e}")


def _assert_ids(codes, w, wav, what):
    """Ids of a path that returns no embeddings: equal where the oracle's margins allow nothing else, else equal or explained."""
    ref, margins = R.acoustic_encode(w, wav, AR.N_Q, return_margins=True)
    assert tuple(codes.shape) == tuple(ref.shape) and codes.dtype == torch.int16
    if float(margins.min()) >= P.RVQ_TIE:
        assert torch.equal(codes.cpu(), ref), f"{what}: ids differ from the oracle"
    else:
        P.assert_rvq_equal_or_explained(codes.cpu(), ref, margins, P.RVQ_TIE, what)
    return float(margins.min())


def test_short_stream_flush_matches_oracle(families):
    """A stream whose whole content is 1000 samples (T = 4): two pushes return nothing, flush() is one final call and returns the oracle's ids."""
    w, enc = families["uniform"]
    N = 1000
    wav = torch.from_numpy(W.synth_waveform(2, N, 24000, seed=8002))
    _, margins = R.acoustic_encode(w, wav, AR.N_Q, return_margins=True)
    assert float(margins.min()) >= P.RVQ_TIE, "choose another seed: this clip must leave the bar nothing to explain"   # 8.3e-2 with this one
    st = enc.new_stream(2)
    a = st.push(wav[:, :600])
    b = st.push(wav[:, 600:])
    assert a.shape[-1] == 0 and b.shape[-1] == 0
    codes = st.flush()
    assert enc.last_status() == 0
    assert tuple(codes.shape) == (2, AR.N_Q, 4) and st.frames_emitted == 4
    _assert_ids(codes, w, wav, "1000-sample stream")


@pytest.mark.parametrize("N", (321, 1000, 1920))
def test_short_clip_through_audiotoken_and_plain_c_entry(N, families):
    """T = 2..6 through AudioToken.encode (numpy [1, N] in, CPU ids out) and through at_encodec_encode, the entry point without a status word."""
    from audiotoken_amd import AudioToken, Tokenizers
    w, enc = families["uniform"]
    wav = AR.waveform(N, 1)
    tok = AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=AR.N_Q, weights=w)
    codes = tok.encode(wav)
    assert codes.device.type == "cpu"
    _assert_ids(codes, w, torch.from_numpy(wav), f"AudioToken.encode N={N}")
    lib, h = enc._h.lib, enc._h.handle
    x = torch.from_numpy(wav).cuda()
    T = AR.chain(N)[4]
    out = torch.full((1, AR.N_Q, T), -1, dtype=torch.int16, device="cuda")
    nbytes = lib.at_encodec_workspace_bytes(h, 1, N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    t_out = C.c_int(0)
    rc = lib.at_encodec_encode(h, x.data_ptr(), None, 1, N, AR.N_Q, out.data_ptr(), C.byref(t_out), None, ws.data_ptr(), nbytes,
                               _cabi.current_stream_handle(torch.device("cuda:0")))
    assert rc == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert t_out.value == T
    _assert_ids(out, w, torch.from_numpy(wav), f"at_encodec_encode N={N}")
