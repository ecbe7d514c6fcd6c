"""CPU: the bookkeeping of the stream pools (audiotoken_amd/streaming.py: AcousticStreamPool, AcousticDecodeStreamPool) with stub device calls, the four
C-ABI additions, and the tick planners of the streamed file drivers.

The stub device: the state of a stream is ONE counter, the number of frames it has emitted. ``gather`` / ``scatter`` move counters between a pool of
``S`` of them and the staging lists, exactly as the library moves state rows. The stub push writes, for frame t of row b, code 0 = counter of the row + t
(the stream's own frame index if its state was routed correctly) and code 1 = the value of the row's first sample of that frame (which stream's samples
these are: stream k pushes samples of value k).
"""
import os
import re

import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd.streaming import FIRST_PUSH_FRAMES, HOP, AcousticDecodeStreamPool, AcousticStreamPool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOL_SYMBOLS = ("at_encodec_stream_gather", "at_encodec_stream_scatter", "at_encodec_decode_stream_gather", "at_encodec_decode_stream_scatter")


class StubOwner:
    """What fallback.encodec_ladder reads: a queue of status words (0 when empty), options, counters."""
    RANGE_OPTIONS = ("ih_f16x2",)

    def __init__(self):
        self.statuses = []
        self.options = {"lstm_pipe": 1, "persistent_lstm": 1, "ih_f16x2": 1}
        self.fallback_batches = 0
        self.nonfinite_batches = 0

    def last_status(self):
        return self.statuses.pop(0) if self.statuses else 0

    def get_option(self, name):
        return self.options[name]

    def set_option(self, name, value):
        self.options[name] = value


class StubDevice:
    def __init__(self, S):
        self.S = S
        self.pool = [0] * S
        self.staging_in, self.staging_out = [], []
        self.log = []          # ("gather" | "scatter", slots) and ("push", B, frames, final, started) in call order

    def gather(self, slots):
        assert len(set(slots)) == len(slots) and all(0 <= s < self.S for s in slots)
        self.log.append(("gather", tuple(slots)))
        self.staging_in = [self.pool[s] for s in slots]

    def scatter(self, slots):
        assert len(set(slots)) == len(slots) and all(0 <= s < self.S for s in slots) and len(slots) == len(self.staging_out)
        self.log.append(("scatter", tuple(slots)))
        for b, s in enumerate(slots):
            self.pool[s] = self.staging_out[b]

    def _advance(self, B, T, started):
        if not started:
            self.staging_in = [0] * B      # the reset of the staging state
        assert len(self.staging_in) == B
        self.staging_out = [c + T for c in self.staging_in]   # staging_in stays as it is: a repeat starts from it
        return torch.tensor(self.staging_in)[:, None] + torch.arange(T)[None]

    def push_encode(self, x, final, started):
        B, n = x.shape
        T = -(-n // HOP)
        self.log.append(("push", B, T, final, started))
        codes = torch.zeros((B, 2, T), dtype=torch.int16)
        codes[:, 0] = self._advance(B, T, started)
        codes[:, 1] = x[:, ::HOP][:, :T].to(torch.int16)
        return codes

    def push_decode(self, tokens, started):
        B, K, t = tokens.shape
        self.log.append(("push", B, t, K, started))
        idx = self._advance(B, t, started)
        # "audio": sample 320 f + i of a row = 1000 * (frame index by the state) + the frame's first token
        return (1000.0 * idx + tokens[:, 0, :]).float().repeat_interleave(HOP, dim=1)

    def pushes(self):
        return [e for e in self.log if e[0] == "push"]


def _enc_pool(S, owner=None):
    dev = StubDevice(S)
    return AcousticStreamPool(None, S, push_fn=dev.push_encode, gather_fn=dev.gather, scatter_fn=dev.scatter, owner=owner, n_q=2), dev


def _drive(pool, totals, chunks):
    """Streams of totals[k] samples of value k + 1, fed chunks[k] samples per tick; a stream is opened when a slot is free, flushed when its samples are
    exhausted. Returns {k: codes [2, T]} and the number of ticks."""
    todo = list(range(len(totals)))
    live, pos, got = {}, {}, {k: [] for k in todo}   # live: sid -> k
    ticks = 0
    while todo or live:
        while todo and len(pool.live) < pool.slots:
            k = todo.pop(0)
            live[pool.open()] = k
            pos[k] = 0
        feed = {}
        for sid, k in live.items():
            n = min(chunks[k], totals[k] - pos[k])
            feed[sid] = torch.full((n,), float(k + 1))
            pos[k] += n
        for sid, c in pool.push(feed).items():
            got[live[sid]].append(c)
        done = [sid for sid, k in live.items() if pos[k] >= totals[k]]
        if done:
            for sid, c in pool.flush(done).items():
                got[live.pop(sid)].append(c)
        ticks += 1
    return {k: torch.cat(v, dim=-1) for k, v in got.items()}, ticks


# 7 streams through 3 slots, ragged: below one frame per tick, exactly 7 frames, frame-aligned and not, several chunks
TOTALS = [321, 2240, 2560, 2561, 7000, 12800, 20013]
CHUNKS = [2560, 2560, 2560, 2560, 1000, 2560, 4000]


def test_every_stream_receives_its_own_frames_in_order():
    pool, dev = _enc_pool(3)
    got, _ = _drive(pool, TOTALS, CHUNKS)
    for k, total in enumerate(TOTALS):
        T = -(-total // HOP)
        assert got[k].shape == (2, T), (k, got[k].shape)
        assert got[k][0].tolist() == list(range(T)), f"stream {k}: frames out of order, missing, or another stream's state"
        assert set(got[k][1].tolist()) == {k + 1}, f"stream {k} received another stream's samples"
    assert pool.live == [] and pool.library_pushes == len(dev.pushes())
    alone = 0
    for k in range(len(TOTALS)):                      # the same clips one at a time: the library pushes a pool of one slot needs
        one, _ = _enc_pool(1)
        _drive(one, TOTALS[k:k + 1], CHUNKS[k:k + 1])
        alone += one.library_pushes
    assert pool.library_pushes < alone, f"rows were never batched: {pool.library_pushes} pushes against {alone} one at a time"


def test_groups_one_push_per_phase_and_length_in_id_order():
    pool, dev = _enc_pool(4)
    a, b, c, d = (pool.open() for _ in range(4))
    assert (a, b, c, d) == (0, 1, 2, 3) and pool.live == [0, 1, 2, 3]
    x = lambda n, v=1.0: torch.full((n,), v)
    # tick 1: a and c start with 8 frames, b with 7, d holds (6 frames < 7)
    out = pool.push({a: x(2560), b: x(2240 + 100), c: x(2560 + 319), d: x(1920)})
    assert [o.shape[-1] for o in (out[a], out[b], out[c], out[d])] == [8, 7, 8, 0]
    assert dev.log == [("push", 2, 8, False, False), ("scatter", (0, 2)), ("push", 1, 7, False, False), ("scatter", (1,))]
    dev.log.clear()
    # tick 2: b (held 100) and c (held 319) both reach 1 frame with 300 more; a gets 2 frames; d starts with its 6 held + 2 = 8 frames
    out = pool.push({d: x(640), c: x(300), b: x(300), a: x(640)})
    assert [out[i].shape[-1] for i in (a, b, c, d)] == [2, 1, 1, 8]
    assert dev.log == [("gather", (0,)), ("push", 1, 2, False, True), ("scatter", (0,)),
                       ("gather", (1, 2)), ("push", 2, 1, False, True), ("scatter", (1, 2)),
                       ("push", 1, 8, False, False), ("scatter", (3,))]
    assert out[b][0].tolist() == [7] and out[c][0].tolist() == [8] and out[a][0].tolist() == [8, 9]
    dev.log.clear()
    # flush: groups by (started, exact held samples); b holds 80, c holds 299, a and d hold nothing (no push, empty output)
    out = pool.flush({a, b, c, d})
    assert [out[i].shape[-1] for i in (a, b, c, d)] == [0, 1, 1, 0]
    assert dev.log == [("gather", (1,)), ("push", 1, 1, True, True), ("gather", (2,)), ("push", 1, 1, True, True)], "a final push is not scattered"
    assert pool.live == []


def test_slots_are_reused_and_a_full_pool_raises():
    pool, dev = _enc_pool(2)
    a, b = pool.open(), pool.open()
    with pytest.raises(RuntimeError, match="slots are in use"):
        pool.open()
    pool.push({a: torch.ones(2560), b: torch.ones(2560)})
    pool.close(a)
    assert pool.live == [b]
    c = pool.open()                                   # slot 0 again, whose counter still says 8: a new stream must not inherit it
    assert c == 2 and pool._rows[c].slot == 0
    out = pool.push({c: torch.ones(2240), b: torch.ones(320)})
    assert out[c][0].tolist() == list(range(7)) and out[b][0].tolist() == [8]
    pool.flush(b)
    d = pool.open()
    assert pool._rows[d].slot == 1 and pool.live == [c, d]
    with pytest.raises(RuntimeError, match="after flush"):
        pool.push({b: torch.ones(320)})
    with pytest.raises(RuntimeError, match="after flush"):
        pool.flush(a)
    with pytest.raises(KeyError):
        pool.push({99: torch.ones(320)})


def test_one_shot_flush_of_a_stream_that_never_started():
    pool, dev = _enc_pool(2)
    a, b = pool.open(), pool.open()
    assert pool.push({a: torch.ones(321), b: torch.ones(321)})[a].shape == (2, 0)
    out = pool.flush([a, b])
    assert dev.log == [("push", 2, 2, True, False)] and out[a][0].tolist() == [0, 1]


def test_a_failed_push_is_repeated_and_scattered_once():
    owner = StubOwner()
    pool, dev = _enc_pool(3, owner)
    a, b = pool.open(), pool.open()
    pool.push({a: torch.ones(2560), b: torch.ones(2560)})
    dev.log.clear()
    before = list(dev.pool)
    owner.statuses = [2]                              # the next status read reports an fp16 range overflow, the one after that 0
    out = pool.push({a: torch.ones(640), b: torch.ones(640)})
    assert dev.log == [("gather", (0, 1)), ("push", 2, 2, False, True), ("push", 2, 2, False, True), ("scatter", (0, 1))]
    assert owner.fallback_batches == 1 and pool.fallback_batches == 1 and pool.library_pushes == 2
    assert owner.options["ih_f16x2"] == 1, "the range fallback must not outlive the push"
    assert out[a][0].tolist() == [8, 9] and dev.pool[:2] == [before[0] + 2, before[1] + 2]
    # a push that fails twice raises and never reaches the pool
    dev.log.clear()
    owner.statuses = [2, 2, 2]
    with pytest.raises(_cabi.HipLibraryError):
        pool.push({a: torch.ones(320)})
    assert not [e for e in dev.log if e[0] == "scatter"] and dev.pool[0] == before[0] + 2
    out = pool.push({a: torch.ones(320)})             # the stream goes on from where it was (the caller pushes the refused samples again)
    assert out[a][0].tolist() == [10]


def test_decode_pool_groups_by_phase_K_and_frames():
    dev = StubDevice(3)
    pool = AcousticDecodeStreamPool(None, 3, push_fn=dev.push_decode, gather_fn=dev.gather, scatter_fn=dev.scatter)
    a, b, c = pool.open(), pool.open(), pool.open()
    tok = lambda K, t, v: torch.full((K, t), v, dtype=torch.long)
    out = pool.push({a: tok(2, 8, 1), b: tok(8, 8, 2), c: tok(2, 3, 3)})
    assert out[a].shape == (8 * HOP,) and out[c].shape == (0,)
    assert dev.log == [("push", 1, 8, 2, False), ("scatter", (0,)), ("push", 1, 8, 8, False), ("scatter", (1,))]
    dev.log.clear()
    out = pool.push({a: tok(2, 4, 1), b: tok(8, 4, 2), c: tok(2, 4, 3)})       # c starts with 3 + 4 = 7 frames
    assert dev.log == [("gather", (0,)), ("push", 1, 4, 2, True), ("scatter", (0,)), ("gather", (1,)), ("push", 1, 4, 8, True), ("scatter", (1,)),
                       ("push", 1, 7, 2, False), ("scatter", (2,))]
    assert out[a][::HOP].tolist() == [8001.0, 9001.0, 10001.0, 11001.0] and out[c][::HOP].tolist() == [1000.0 * f + 3 for f in range(7)]
    dev.log.clear()
    out = pool.push({a: tok(2, 5, 1), c: tok(2, 5, 3)})                        # same phase, K and frames: one push of B = 2
    assert dev.log == [("gather", (0, 2)), ("push", 2, 5, 2, True), ("scatter", (0, 2))]
    assert out[c][::HOP].tolist() == [1000.0 * f + 3 for f in range(7, 12)]
    assert pool.flush({a, b, c})[a].shape == (0,) and pool.live == []
    d = pool.open()
    pool.push({d: tok(2, 3, 4)})
    dev.log.clear()
    pool.flush(d)                                     # never started: what it holds goes to the library, which rules on T < 7
    assert dev.pushes() == [("push", 1, 3, 2, False)] and FIRST_PUSH_FRAMES == 7


def test_facade_pools_are_acoustic_only(tmp_path):
    from audiotoken_amd import AudioToken, Tokenizers
    for t in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        tok = AudioToken(t, device="cuda:0")                    # nothing is loaded before the refusal
        with pytest.raises(ValueError, match="acoustic only"):
            tok.stream_pool(4)
        with pytest.raises(ValueError, match="acoustic only"):
            tok.decode_stream_pool(4)
        with pytest.raises(ValueError, match="acoustic only"):
            tok.encode_batch_files(batch_size=2, outdir=tmp_path, audio_files=["a.wav"], stream=True)
        assert tok.encoder is None and tok.decoder is None


# ---- the tick planners of the streamed file drivers (audiotoken_amd/writer.py) -------------------------------------------------------------------------------
def _ticks(it):
    return [[(r.file, r.t0, r.valid, r.last) for r in tick] for tick in it]


def test_decode_tick_plan_on_hand_written_cases():
    from audiotoken_amd.writer import plan_stream_ticks
    # a file shorter than one chunk, a file of exactly 2 chunks, one of 2 chunks and a frame, mixed K; 2 places
    files = [(8, 10), (2, 150), (8, 151), (2, 3)]
    assert _ticks(plan_stream_ticks(files, 2, 75)) == [
        [(0, 0, 10, True), (1, 0, 75, False)],
        [(1, 75, 75, True), (2, 0, 75, False)],                     # file 0 left with tick 0: its place went to file 2
        [(2, 75, 75, False), (3, 0, 3, True)],
        [(2, 150, 1, True)]]
    # batch_size larger than the file count: everything is live from the first tick on
    assert _ticks(plan_stream_ticks(files, 16, 75)) == [
        [(0, 0, 10, True), (1, 0, 75, False), (2, 0, 75, False), (3, 0, 3, True)],
        [(1, 75, 75, True), (2, 75, 75, False)],
        [(2, 150, 1, True)]]
    # no chunking: every file is one row; one place: one file after the other
    assert _ticks(plan_stream_ticks(files[:2], 4, None)) == [[(0, 0, 10, True), (1, 0, 150, True)]]
    assert _ticks(plan_stream_ticks(files[:2], 1, 100)) == [[(0, 0, 10, True)], [(1, 0, 100, False)], [(1, 100, 50, True)]]
    assert _ticks(plan_stream_ticks([], 4, 75)) == []


def test_tick_plan_reads_the_next_file_only_when_a_place_is_free():
    from audiotoken_amd.writer import plan_stream_ticks
    seen = []

    def files():
        for i, kt in enumerate([(8, 200), (8, 100), (8, 50)]):
            seen.append(i)
            yield kt

    it = plan_stream_ticks(files(), 2, 100)
    next(it)
    assert seen == [0, 1], "the third file was opened while both places were taken"
    assert _ticks([next(it)]) == [[(0, 100, 100, True), (2, 0, 50, True)]] and seen == [0, 1, 2]


def test_encode_tick_plan_on_hand_written_cases():
    from audiotoken_amd.writer import plan_encode_stream_ticks
    # per file the sample counts of its chunks: shorter than one chunk, exactly 2 chunks, 3 chunks with a 2-sample tail
    files = [[12000], [24000, 24000], [24000, 24000, 2]]
    assert _ticks(plan_encode_stream_ticks(files, 2)) == [
        [(0, 0, 1, True), (1, 0, 1, False)],
        [(1, 1, 1, True), (2, 0, 1, False)],
        [(2, 1, 1, False)],
        [(2, 2, 1, True)]]
    assert _ticks(plan_encode_stream_ticks(files, 8)) == [
        [(0, 0, 1, True), (1, 0, 1, False), (2, 0, 1, False)], [(1, 1, 1, True), (2, 1, 1, False)], [(2, 2, 1, True)]]


# ---- the C ABI additions ---------------------------------------------------------------------------------------------------------------------------
def test_pool_symbols_are_declared_bound_and_exported():
    text = open(os.path.join(ROOT, "include", "audiotoken_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    lib = _cabi.load()
    for s in POOL_SYMBOLS:
        assert re.search(r"\bint\s+" + s + r"\s*\(", text), f"{s} is not declared in include/audiotoken_hip.h"
        assert s in _cabi.SIGNATURES and len(_cabi.SIGNATURES[s][1]) == 8, f"{s} is not bound in _cabi.py"
        assert hasattr(lib, s), f"{s} is not exported"


def test_pool_calls_refuse_a_null_handle_without_a_device():
    lib = _cabi.load()
    slots = (_cabi.C.c_int32 * 1)(0)
    for s in POOL_SYMBOLS:
        args = (None, None, 1, None, slots, 1, None, None) if s.endswith("gather") else (None, None, 1, None, slots, None, 1, None)
        assert getattr(lib, s)(*args) != 0
        assert "not finalized" in _cabi.last_error()
