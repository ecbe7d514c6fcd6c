"""GPU: stream pools (at_encodec_*stream_gather / _scatter, AcousticStreamPool, AcousticDecodeStreamPool).

The bar.
* The state copies are exact: raw bytes, torch.equal.
* The same groups give the same bits: streams that go through a pool in lockstep are one lockstep stream of that B plus two exact copies per push, so codes,
  embeddings and audio are asserted torch.equal to AcousticStream(batch) / AcousticDecodeStream(batch) on the same schedule.
* Ragged encode rows: every clip's tokens torch.equal the one-shot tokens of that clip alone on the same handle (the contract of tests/test_stream_gpu.py)
  and meet the oracle bar of tests/parity.py (embeddings within FLOAT_TOL, ids equal or explained by an oracle near-tie).
* Ragged decode rows: every file's audio within the decode bar of tests/test_stream_decode_gpu.py (max abs < 1e-3, relative L2 < 1e-4) of the one-shot decode
  of that file and of the B = 1 AcousticDecodeStream on the same schedule. A pooled row of a group of B > 1 runs the B = 1 stream's arithmetic on other tiles
  (the GEMMs see another M), so equality of bits with the B = 1 stream is printed, not asserted.
"""
import functools

import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import weights as W
from audiotoken_amd.streaming import HOP
from oracle import encodec_ref as R
from tests import parity as P

pytestmark = pytest.mark.gpu

ABS_BAR, REL_BAR = 1e-3, 1e-4     # tests/test_stream_decode_gpu.py's (test_decode_matches_golden's)
ENC_PLANES = (640, 512, 512, 512, 512, 6 * 512)     # ctx, h0, c0, h1, c1, yhist (floats per stream)
DEC_PLANES = (6 * 128, 512, 512, 512, 512, 2 * 512)  # zhist, h0, c0, h1, c1, yctx


@pytest.fixture(scope="module")
def enc_weights():
    return W.synth_encodec_weights(seed=0, with_decoder=False)


@pytest.fixture(scope="module")
def dec_weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True, family="trained_like")


def _encoder(weights, n_q=8):
    from audiotoken_amd.configs import AcousticEncoderConfig
    from audiotoken_amd.encoder import AcousticEncoder
    return AcousticEncoder(AcousticEncoderConfig(bandwidth={2: 1.5, 4: 3, 8: 6}[n_q]), device="cuda:0", weights=weights)


def _decoder(weights):
    from audiotoken_amd.configs import AcousticDecoderConfig
    from audiotoken_amd.decoder import AcousticDecoder
    return AcousticDecoder(AcousticDecoderConfig(), device="cuda:0", weights=weights)


@pytest.fixture(scope="module")
def encoders(cuda_device, enc_weights):
    return {nq: _encoder(enc_weights, nq) for nq in (2, 8)}


@pytest.fixture(scope="module")
def decoder(cuda_device, dec_weights):
    return _decoder(dec_weights)


@functools.lru_cache(maxsize=None)
def _wav(B, total, seed):
    return torch.from_numpy(W.synth_waveform(B, total, 24000, seed=seed))


@functools.lru_cache(maxsize=None)
def _tokens(K, T, seed):
    return torch.randint(0, 1024, (K, T), dtype=torch.long, generator=torch.Generator().manual_seed(9000 + 17 * K + T + seed))


# ---- 1. the state copies are exact -------------------------------------------------------------------------------------------------------------------
class _Side:
    """One direction's five entry points on a model's handle."""

    def __init__(self, model, decode):
        self.lib, self.h, self.dev = model._h.lib, model._h.handle, model.device
        p = "at_encodec_decode_stream" if decode else "at_encodec_stream"
        self.bytes_fn, self.reset_fn = getattr(self.lib, p + "_state_bytes"), getattr(self.lib, p + "_reset")
        self.gather_fn, self.scatter_fn = getattr(self.lib, p + "_gather"), getattr(self.lib, p + "_scatter")
        self.planes = DEC_PLANES if decode else ENC_PLANES

    def state(self, B, reset=True):
        t = torch.empty(self.bytes_fn(self.h, B), dtype=torch.uint8, device=self.dev)
        if reset:
            assert self.reset_fn(self.h, t.data_ptr(), B, _cabi.current_stream_handle(self.dev)) == 0
        return t

    def _slots(self, slots):
        host = torch.tensor(slots, dtype=torch.int32)
        return host, host.to(self.dev)

    def gather(self, pool, S, slots, B, out, dev_slots=True, host_slots=True):
        host, dev = self._slots(slots)
        return self.gather_fn(self.h, _cabi.ptr(pool), S, dev.data_ptr() if dev_slots else 0, host.data_ptr() if host_slots else 0, B, _cabi.ptr(out),
                              _cabi.current_stream_handle(self.dev))

    def scatter(self, state, B, slots, pool, S):
        host, dev = self._slots(slots)
        return self.scatter_fn(self.h, _cabi.ptr(state), B, dev.data_ptr(), host.data_ptr(), _cabi.ptr(pool), S, _cabi.current_stream_handle(self.dev))

    def rows(self, state, R_):
        """The state of R_ streams as a list of per-plane int32 views [R_, w]."""
        words, out, off = state.view(torch.int32), [], 0
        for w in self.planes:
            out.append(words[off:off + R_ * w].view(R_, w))
            off += R_ * w
        assert off == words.numel()
        return out


def _fill(side, S, seed):
    pool = side.state(S)
    pattern = torch.randint(0, 256, (pool.numel(),), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed)).to(side.dev)
    pool.copy_(pattern)   # distinct bit patterns, NaN payloads and denormals among them: a copy must not care
    return pool


@pytest.mark.parametrize("decode", (False, True), ids=("encode", "decode"))
@pytest.mark.parametrize("slots", ([4, 0, 2], [3], [0, 1, 2, 3, 4], [4, 3, 2, 1, 0]), ids=("B3", "B1", "B5", "B5_reversed"))
def test_gather_then_scatter_is_exact(encoders, decoder, decode, slots):
    side = _Side(decoder if decode else encoders[8], decode)
    S, B = 5, len(slots)
    assert side.bytes_fn(side.h, 1) == 4 * sum(side.planes) == (15360 if decode else 23040)
    pool = _fill(side, S, 5 + B)
    keep = pool.clone()
    staging = side.state(B, reset=False)
    staging.fill_(0xA5)
    assert side.gather(pool, S, slots, B, staging) == 0, _cabi.last_error()
    assert torch.equal(pool, keep), "gather wrote to the pool"
    for plane_pool, plane_st in zip(side.rows(pool, S), side.rows(staging, B)):
        assert torch.equal(plane_st, plane_pool[slots]), "row b of the staging state is not row slots[b] of the pool"
    target = side.state(S)                                      # zeroed
    assert side.scatter(staging, B, slots, target, S) == 0, _cabi.last_error()
    others = [s for s in range(S) if s not in slots]
    for plane_pool, plane_t in zip(side.rows(pool, S), side.rows(target, S)):
        assert torch.equal(plane_t[slots], plane_pool[slots]), "scatter did not restore the gathered rows"
        assert not bool(plane_t[others].ne(0).any()), "scatter touched a row outside the slot list"


@pytest.mark.parametrize("decode", (False, True), ids=("encode", "decode"))
def test_argument_errors_leave_the_device_usable(encoders, decoder, decode):
    side = _Side(decoder if decode else encoders[8], decode)
    other = _Side(encoders[8] if decode else decoder, not decode)
    S = 5
    pool, staging = _fill(side, S, 3), side.state(3, reset=False)
    # an address no reset can have noted, whatever the allocator handed out before: allocations are at least 256-byte aligned, this one is 16 bytes past one
    unknown = torch.zeros(pool.numel() + 16, dtype=torch.uint8, device=side.dev)[16:]
    small = side.state(3)                                       # known, but for 3 streams
    if decode:                                                  # an encode pool of the SAME handle (a decoder's handle holds the encoder too)
        wrong_way = torch.empty(other.bytes_fn(side.h, S), dtype=torch.uint8, device=side.dev)
        assert other.reset_fn(side.h, wrong_way.data_ptr(), S, _cabi.current_stream_handle(side.dev)) == 0
    else:                                                       # a decode pool, which only another handle can have reset
        wrong_way = other.state(S)

    def refused(rc, what):
        assert rc != 0, f"{what} was accepted"
        assert _cabi.last_error(), f"{what}: at_last_error is empty"

    refused(side.gather(None, S, [0, 1, 2], 3, staging), "a null pool")
    refused(side.gather(pool, S, [0, 1, 2], 3, None), "a null state")
    refused(side.gather(pool, S, [0, 1, 2], 3, staging, dev_slots=False), "a null device slot list")
    refused(side.gather(pool, S, [0, 1, 2], 3, staging, host_slots=False), "a null host slot list")
    refused(side.gather(pool, S, [0], 0, staging), "B = 0")
    refused(side.gather(pool, S, [0, 1, 2, 3, 4, 0], 6, staging), "B > S")
    refused(side.gather(pool, S, [0, 5, 2], 3, staging), "slot S")
    refused(side.gather(pool, S, [0, -1, 2], 3, staging), "slot -1")
    refused(side.gather(pool, S, [2, 0, 2], 3, staging), "a duplicate slot")
    refused(side.gather(unknown, S, [0, 1, 2], 3, staging), "a pool the handle never reset")
    refused(side.gather(small, S, [0, 1, 2], 3, staging), "a pool reset for another S")
    refused(side.gather(wrong_way, S, [0, 1, 2], 3, staging), "a pool of the other direction")
    refused(side.gather(pool, S, [0, 1, 2], 3, pool), "state == pool")
    refused(side.scatter(unknown, 3, [0, 1, 2], pool, S), "scatter from a state the handle does not know")
    refused(side.scatter(small, 2, [0, 1], pool, S), "scatter from a state of another B")
    refused(side.scatter(pool, S, [0, 1, 2, 3, 4], pool, S), "scatter with state == pool")
    # nothing was launched, and a valid call works
    keep = pool.clone()
    assert side.gather(pool, S, [4, 0, 2], 3, staging) == 0, _cabi.last_error()
    torch.cuda.synchronize()
    assert torch.equal(pool, keep)
    assert all(torch.equal(a, b[[4, 0, 2]]) for a, b in zip(side.rows(staging, 3), side.rows(pool, S)))


def test_scatter_from_a_finished_stream_is_refused(encoders):
    enc = encoders[8]
    side = _Side(enc, False)
    st = enc.new_stream(1)
    st.push(_wav(1, 2561, 1).cuda())
    st.flush()                                                  # a final push of one sample: the state it wrote is noted as finished, its input is not
    pool = side.state(5)
    finished = [s for s in st._state if side.scatter(s, 1, [0], pool, 5) != 0]
    assert len(finished) == 1 and "finished" in _cabi.last_error()


# ---- 2. same groups, same bits -----------------------------------------------------------------------------------------------------------------------
def test_lockstep_through_a_pool_equals_the_lockstep_stream(encoders):
    enc = encoders[8]
    total = 45 * HOP
    x = _wav(3, total, 1003).cuda()
    st = enc.new_stream(3)
    st.keep_embeddings = True
    pool = enc.new_stream_pool(slots=5)
    pool.keep_embeddings = True
    pool.open()
    ids = [pool.open(), pool.open()]
    pool.close(0)
    ids.append(pool.open())                                     # ids 1, 2, 3 in slots 1, 2, 0: the rows of a group are not its slots
    for pos in range(0, total, 6400):
        ref = st.push(x[:, pos:pos + 6400])
        got = pool.push({sid: x[b, pos:pos + 6400] for b, sid in enumerate(ids)})
        assert all(torch.equal(got[sid], ref[b]) for b, sid in enumerate(ids)), f"codes differ at sample {pos}"
        assert all(torch.equal(pool.last_embeddings[sid], st.last_embeddings[b]) for b, sid in enumerate(ids)), f"embeddings differ at sample {pos}"
    ref, got = st.flush(), pool.flush(ids)
    assert all(torch.equal(got[sid], ref[b]) for b, sid in enumerate(ids))
    assert pool.library_pushes == 3 and pool.live == []         # 20 + 20 + 5 frames; the stream ends on a frame boundary


def test_decode_lockstep_through_a_pool_equals_the_lockstep_stream(decoder):
    toks = torch.stack([_tokens(8, 45, b) for b in range(3)]).cuda()
    st = decoder.new_stream(3)
    pool = decoder.new_stream_pool(slots=5)
    pool.open()
    ids = [pool.open() for _ in range(3)]
    pool.close(0)                                               # slots 1, 2, 3
    for pos in range(0, 45, 20):
        ref = st.push(toks[:, :, pos:pos + 20])
        got = pool.push({sid: toks[b, :, pos:pos + 20] for b, sid in enumerate(ids)})
        assert all(torch.equal(got[sid], ref[b]) for b, sid in enumerate(ids)), f"audio differs at frame {pos}"
    assert all(v.numel() == 0 for v in pool.flush(ids).values()) and pool.library_pushes == 3


# ---- 3. ragged rows --------------------------------------------------------------------------------------------------------------------------------
CLIPS = (321, 2240, 2560, 2561, 7000, 12800, 20013)
CHUNK = 8 * HOP

_ENC_ORACLE = {}


def _enc_oracle(weights, k, n_q):
    if k not in _ENC_ORACLE:
        _ENC_ORACLE[k] = R.seanet_encode(weights, _wav(1, CLIPS[k], 2000 + k))
    if (k, n_q) not in _ENC_ORACLE:
        codes, margins = R.rvq_encode(weights, _ENC_ORACLE[k], n_q, return_margins=True)
        _ENC_ORACLE[(k, n_q)] = (codes.transpose(0, 1).to(torch.int16), margins.transpose(0, 1))
    return (_ENC_ORACLE[k].permute(0, 2, 1).contiguous(),) + _ENC_ORACLE[(k, n_q)]


def _feed_through_pool(pool, clips, chunk, length, piece, take):
    """clips fed `chunk` units per tick through the pool, a clip opened when a slot is free, flushed when exhausted; take(k, output dict entry)."""
    todo, live, pos = list(range(len(clips))), {}, {}
    while todo or live:
        while todo and len(pool.live) < pool.slots:
            k = todo.pop(0)
            live[pool.open()] = k
            pos[k] = 0
        feed = {}
        for sid, k in live.items():
            feed[sid] = piece(clips[k], pos[k], pos[k] + chunk)
            pos[k] += chunk
        for sid, out in pool.push(feed).items():
            take(live[sid], sid, out)
        done = [sid for sid, k in live.items() if pos[k] >= length(clips[k])]
        if done:
            res = pool.flush(done)
            for sid in done:
                take(live.pop(sid), sid, res[sid])


@pytest.mark.parametrize("n_q", (2, 8))
def test_ragged_encode_rows(encoders, enc_weights, n_q):
    enc = encoders[n_q]
    clips = [_wav(1, n, 2000 + k)[0].cuda() for k, n in enumerate(CLIPS)]
    pool = enc.new_stream_pool(slots=3)
    pool.keep_embeddings = True
    codes, embs = {k: [] for k in range(len(clips))}, {k: [] for k in range(len(clips))}

    def take(k, sid, out):
        if out.shape[-1]:
            codes[k].append(out.clone())
            embs[k].append(pool.last_embeddings[sid].clone())

    _feed_through_pool(pool, clips, CHUNK, lambda c: c.shape[0], lambda c, a, b: c[a:b], take)
    assert enc.last_status() == 0 and pool.live == []
    alone = 0
    for k, x in enumerate(clips):
        what = f"n_q {n_q}, clip of {CLIPS[k]} samples"
        got, emb = torch.cat(codes[k], dim=-1), torch.cat(embs[k], dim=0)
        one = enc(x[None], None)
        assert enc.last_status() == 0
        assert got.shape == one[0].shape == (n_q, -(-CLIPS[k] // HOP))
        assert torch.equal(got, one[0]), f"{what}: {int((got != one[0]).sum())} token ids differ from the one-shot encode of the clip alone"
        emb_ref, codes_ref, margins = _enc_oracle(enc_weights, k, n_q)
        err = (emb.cpu()[None] - emb_ref).abs().max().item()
        print(f"{what}: max |pool - oracle| embedding difference {err:.3e}")
        assert err < P.FLOAT_TOL, f"{what}: embedding differs from the oracle by {err}"
        P.assert_rvq_equal_or_explained(got.cpu()[None], codes_ref, margins, P.RVQ_TIE, what)
        st, n = enc.new_stream(1), 0                            # the same clip alone on the same schedule: how many library pushes that takes
        for pos in range(0, CLIPS[k], CHUNK):
            n += int(st.push(x[None, pos:pos + CHUNK]).shape[-1] > 0)
        n += int(st.flush().shape[-1] > 0)
        alone += n
    print(f"n_q {n_q}: {pool.library_pushes} library pushes through the pool, {alone} one clip at a time")
    assert pool.library_pushes < alone, "rows were never batched"


# (K, frames). The pool groups by (phase, K, frames), so only files of equal K that are live together can share a push: neighbours in the order get the same K
# (K = 2 and K = 8 still meet in one tick: the 9-frame file's last frame beside the two K = 2 files that start). By the grouping rule the three slots then
# need 14 library pushes for the six decodable files where one file at a time needs 1 + 1 + 2 + 3 + 5 + 8 = 20.
DEC_FILES = ((2, 3), (8, 7), (8, 8), (8, 9), (2, 21), (2, 40), (2, 63))


def _close(got, ref, what):
    got, ref = got.cpu().double(), ref.cpu().double()
    err, rel = (got - ref).abs().max().item(), ((got - ref).norm() / ref.norm()).item()
    print(f"{what}: max abs difference {err:.3e}, relative L2 {rel:.3e}, bits equal: {bool(torch.equal(got, ref))}")
    assert err < ABS_BAR and rel < REL_BAR, f"{what}: max abs {err}, relative L2 {rel}"


def test_ragged_decode_rows(decoder):
    from audiotoken_amd._cabi import HipLibraryError
    files = [_tokens(K, T, 50 + i).cuda() for i, (K, T) in enumerate(DEC_FILES)]
    with pytest.raises(HipLibraryError):                        # what one-shot decode says about 3 frames
        decoder(files[0][None])
    pool = decoder.new_stream_pool(slots=3)
    audio = {k: [] for k in range(len(files))}

    def take(k, sid, out):
        audio[k].append(out.clone())

    # the 3-frame file first on its own: its flush raises what one-shot decode raises, and its slot is free afterwards
    sid = pool.open()
    assert pool.push({sid: files[0]})[sid].numel() == 0
    with pytest.raises(HipLibraryError, match="7 frames"):
        pool.flush(sid)
    assert pool.live == []
    _feed_through_pool(pool, files[1:], 8, lambda f: f.shape[-1], lambda f, a, b: f[:, a:b], lambda k, sid, out: take(k + 1, sid, out))
    assert decoder.last_status() == 0 and pool.live == []
    alone = 0
    for k in range(1, len(files)):
        K, T = DEC_FILES[k]
        got = torch.cat(audio[k])
        assert got.shape == (HOP * T,)
        one = decoder(files[k][None]).reshape(-1)
        assert decoder.last_status() == 0
        _close(got, one, f"K {K}, {T} frames, pool vs one-shot decode")
        st, parts = decoder.new_stream(1), []
        for pos in range(0, T, 8):
            parts.append(st.push(files[k][None, :, pos:pos + 8])[0])
            alone += int(parts[-1].numel() > 0)
        parts.append(st.flush()[0])
        alone += int(parts[-1].numel() > 0)
        _close(got, torch.cat(parts), f"K {K}, {T} frames, pool vs the B = 1 stream")
    print(f"{pool.library_pushes} library pushes through the pool, {alone} one file at a time")
    assert pool.library_pushes < alone, "rows were never batched"


# ---- 4. a failed push does not reach the pool ------------------------------------------------------------------------------------------------------------
def test_forced_timeout_in_mid_stream_does_not_reach_the_pool(enc_weights, cuda_device):
    """lstm_spin_limit = 0 makes one mid-stream group push report status 1 (no fault: a bounded wait gives up); the ladder repeats it from the gathered
    staging state on another LSTM route, and only the repeat is scattered. The tokens equal the undisturbed pooled run's."""
    B, total = 20, 45 * HOP
    x = _wav(B, total, 1020).cuda()
    pieces = [(0, 4800), (4800, 9600), (9600, total)]

    def run(enc, disturb):
        pool = enc.new_stream_pool(slots=B)
        ids = [pool.open() for _ in range(B)]
        out = []
        for i, (a, b) in enumerate(pieces):
            if disturb and i == 1:
                enc.set_option("lstm_spin_limit", 0)
            got = pool.push({sid: x[r, a:b] for r, sid in enumerate(ids)})
            if disturb and i == 1:
                assert enc.last_status() == 0 and enc.get_option("lstm_pipe") == 0, "the give-up was not seen and repeated"
                enc.set_option("lstm_spin_limit", 1 << 18)
            out.append(torch.stack([got[sid] for sid in ids]))
        got = pool.flush(ids)
        out.append(torch.stack([got[sid] for sid in ids]))
        return torch.cat(out, dim=-1)

    ref = run(_encoder(enc_weights, 8), False)
    got = run(_encoder(enc_weights, 8), True)
    assert torch.equal(got, ref), f"{int((got != ref).sum())} ids differ from the undisturbed pooled run"
    codes_ref, margins = R.acoustic_encode(enc_weights, _wav(B, total, 1020), 8, return_margins=True)
    P.assert_rvq_equal_or_explained(got.cpu(), codes_ref, margins, P.RVQ_TIE, "pool with a forced hand-off timeout")
