"""GPU: stage 1 of the stream pools (csrc/gpt.hip: at_gpt_pool_push): live streams that open, push and flush on their own share the
GPT's cache rows and ticks, each following §25's rule on its own source with its own draws. The protocol is tests/test_long_form_gpu.py's ``verify_long``
on a view of each stream's kept ids and logits; the sources and draws are tests/gpt_queue_cases.py's, which tests/test_gpt_queue_cpu.py shows do not lean
on the sampling waiver. With one cache row a stream is bit-equal to ``to_acoustic_long([source])``."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audiotoken_amd.semantic_decoder import SemanticToAcoustic
from audiotoken_amd.semantic_pool import pool_max_len, pool_schedule

from tests import gpt_queue_cases as Q
from tests import long_form_cases as K
from tests import semantic_pool_cases as P
from tests.semantic_stream_cases import splittings
from tests.test_long_form_gpu import DEV, decoder, verify_long

pytestmark = pytest.mark.gpu


def new_pool(dec, case, streams, slots, tick_tokens=None):
    return dec.stream_pool(streams=streams, slots=slots, window=case["S"], hop=case["H"], max_new_tokens=case["max_new"], temperature=K.TEMPERATURE,
                           top_k=K.TOP_K, tick_tokens=tick_tokens, keep_ids=True, return_logits=True)


def drive(pool, case, srcs, u, calls, check=True):
    """Run ``calls`` (tests/semantic_pool_cases.py's form) on the pool. After every call the device's trace, rounds and placement must be ``pool_schedule``'s,
    given the final windows' lengths the device produced. Returns (the streams' ids, per call ``(streams, ticks, events)``)."""
    sid, at, log = {}, [0] * len(srcs), []
    for c in calls:
        for i in c["open"]:
            sid[i] = pool.open(uniforms=u[i])
        items = {}
        for i, m in c["push"].items():
            items[sid[i]] = srcs[i][at[i]:at[i] + m]
            at[i] += m
        got = pool.push(items, flush=[sid[i] for i in c["flush"]])
        assert sorted(got) == sorted(set(items) | {sid[i] for i in c["flush"]})
        if not check or not pool.last_call:
            continue
        streams = [(b, m, f) for _, b, m, f in pool.last_call]
        ends = []
        for s, _, _, f in pool.last_call:
            rec = pool.stream(s)
            ends.append(rec.windows[-1][3] + (1 if rec.finish == "stop" else 0) if f else 0)
        rounds, ticks, placement, events = pool_schedule(streams, case["S"], case["H"], K.r, case["block"], case["max_new"], pool.slots, pool.tick_tokens,
                                                         final_steps=ends, detail=True)
        assert pool.last_ticks == ticks and pool.last_rounds == len(rounds) and pool.last_placement == placement
        assert all(1 <= a + c2 <= pool.tick_tokens and route == (1 if a + c2 > 64 else 0) for a, _, c2, route, _ in ticks)
        log.append((pool.last_call, ticks, events, rounds))
    return sid, log


def view(pool, dec, sids):
    """The streams' kept ids and logits as ``verify_long`` takes a result: an ``AcousticGeneration`` and the raw buffer, -1 where nothing was written."""
    recs = [pool.stream(s) for s in sids]
    raw_rows = [torch.cat([pool.ids_of(s), rec.tail.cpu().to(torch.int64)]) for s, rec in zip(sids, recs)]
    raw = torch.full((len(sids), max(len(x) for x in raw_rows)), -1, dtype=torch.int64)
    for b, x in enumerate(raw_rows):
        raw[b, :len(x)] = x
    out = dec._generation([pool.ids_of(s) for s in sids], [rec.finish for rec in recs], [pool.logits_of(s) for s in sids], [rec.windows for rec in recs])
    return out, SimpleNamespace(block_size=dec.block_size, last_raw_ids=raw)


def verify(w, dec, case, pool, sid, srcs, u, rows=None):
    rows = list(range(len(srcs))) if rows is None else rows
    out, raw = view(pool, dec, [sid[i] for i in rows])
    return verify_long(w, raw, K.CFG, [srcs[i] for i in rows], out, u[rows], case["S"], case["H"], case["max_new"])


def round_robin(pieces):
    """Calls in which call c pushes piece c of every stream that still has one; a stream is flushed with its last piece (even i) or in the call after."""
    calls, n = [], len(pieces)
    for c in range(max(len(p) for p in pieces) + 1):
        call = {"open": list(range(n)) if c == 0 else [], "push": {}, "flush": []}
        for i, p in enumerate(pieces):
            if c < len(p):
                call["push"][i] = p[c]
            if (c == len(p) - 1 and i % 2 == 0) or (c == len(p) and i % 2 == 1):
                call["flush"].append(i)
        calls.append(call)
    return calls


@pytest.mark.parametrize("family", K.FAMILIES)
def test_one_slot_is_to_acoustic_long_bit_for_bit_under_every_splitting(family):
    w, dec = decoder(family)
    case = Q.CASES["single"]
    srcs, u = Q.inputs("single")
    alone = [dec.to_acoustic_long([src], window=case["S"], hop=case["H"], max_new_tokens=case["max_new"], temperature=K.TEMPERATURE, top_k=K.TOP_K,
                                  uniforms=u[i:i + 1], return_logits=True) for i, src in enumerate(srcs)]
    for name in ("ones", "random", "at_window", "past_window"):
        pool = new_pool(dec, case, streams=len(srcs), slots=1)
        pieces = [splittings(len(src), case["S"], case["H"], seed=i)[name] for i, src in enumerate(srcs)]
        sid, log = drive(pool, case, srcs, u, round_robin(pieces))
        assert all(a + b == 1 for _, ticks, _, _ in log for a, b, _, _, _ in ticks), "a lone prefill or a lone step"
        for i in range(len(srcs)):
            rec = pool.stream(sid[i])
            assert torch.equal(pool.ids_of(sid[i]), alone[i].ids[0] + K.CFG.ACOUSTIC_OFFSET), (name, i)
            assert rec.finish == alone[i].finish[0] and rec.windows == alone[i].windows[0], (name, i)
            assert torch.equal(pool.logits_of(sid[i]), alone[i].logits[0]), f"{name} stream {i}: logit for logit"
            assert bool((rec.tail == -1).all()), "nothing is written past a stream's length"


MIXED_SEED = 5


@pytest.mark.parametrize("family", K.FAMILIES)
def test_four_slots_twelve_streams_interleaved(family):
    w, dec = decoder(family)
    case = Q.CASES["mixed"]
    srcs, u = Q.inputs("mixed")
    calls = P.interleaving(case["lens"], MIXED_SEED, most=6, late=(11,), width=(4, 9))
    pool = new_pool(dec, case, streams=12, slots=4)
    sid, log = drive(pool, case, srcs, u, calls)
    verify(w, dec, case, pool, sid, srcs, u)
    flushed_at = {i: c for c, call in enumerate(calls) for i in call["flush"]}
    opened_at = {i: c for c, call in enumerate(calls) for i in call["open"]}
    assert opened_at[11] > min(flushed_at.values()), "a stream opened after another was flushed"
    assert any(opened_at[j] <= flushed_at[i] < flushed_at[j] and any(j in c["push"] for c in calls[flushed_at[i] + 1:])
               for i in flushed_at for j in flushed_at), "a stream is flushed while another is mid-source"
    assert any(a >= 2 and b >= 1 for _, ticks, _, _ in log for a, b, _, _, _ in ticks), "a tick with two step rows and a prefill"
    # a window waited for a row: more streams had windows in a round than there are rows
    assert any(sum(1 for x in rd if x is not None and (x[3] or x[4])) > 4 for _, _, _, rounds in log for rd in rounds)
    beside = False
    for _, _, events, _ in log:
        final_in = {}
        for steps, starts, _, _ in events:
            for j, _, _, _, fin in starts:
                final_in[j] = fin
            kinds = {final_in[j] for j, _, _ in steps} | {fin for *_, fin in starts}
            beside = beside or kinds == {True, False}
    assert beside, "a final window ran beside non-final ones"


def test_both_routes():
    case = Q.CASES["routes"]
    w, dec = decoder("peaky", block=128)
    srcs, u = Q.inputs("routes")
    calls = P.interleaving(case["lens"], 9, most=20, width=(6, 12))
    pool = new_pool(dec, case, streams=len(srcs), slots=8)
    sid, log = drive(pool, case, srcs, u, calls)
    routes = {route for _, ticks, _, _ in log for *_, route, _ in ticks}
    assert routes == {0, 1}, "ticks on the GEMM route (more than 64 tokens) and on the step kernel"
    assert any(a > 0 and c > 0 and route == 1 for _, ticks, _, _ in log for a, _, c, route, _ in ticks), "a mixed tick on the GEMM route"
    verify(w, dec, case, pool, sid, srcs, u)


def test_stop_heavy_streams_hand_their_rows_on_at_polls():
    case = Q.CASES["stop"]
    w = Q.stop_heavy_weights()
    dec = SemanticToAcoustic(K.CFG, device=DEV, weights=w)
    srcs, u = Q.inputs("stop")
    n = len(srcs)
    calls = [{"open": list(range(n)), "push": {i: len(s) for i, s in enumerate(srcs)}, "flush": []}, {"open": [], "push": {}, "flush": list(range(n))}]
    pool = new_pool(dec, case, streams=n, slots=2)
    sid, log = drive(pool, case, srcs, u, calls)
    verify(w, dec, case, pool, sid, srcs, u)
    assert [pool.stream(sid[i]).finish for i in range(n)] == ["stop"] * n
    last_call, ticks, events, _ = log[-1]
    place = pool.last_placement
    budgets = [min(case["max_new"], case["block"] - pool.stream(s).windows[-1][1] - 1 - pool.stream(s).windows[-1][2]) for s, *_ in last_call]
    early = [x for x, (s, *_) in enumerate(last_call) if pool.stream(s).windows[-1][3] + 1 < budgets[x]]
    assert [x for x in early if (place[x][2] + 1) % 16 == 0], "a stream that stops inside its budget hands its row on at a poll"
    assert any(polled for _, _, polled, _ in events)


def test_one_long_push_beside_short_ones_is_absorbed_in_global_rounds():
    w, dec = decoder("peaky")
    S, H = K.S, K.H
    case = dict(S=S, H=H, block=K.BLOCK, max_new=K.MAX_NEW)
    lens = [5 * S, 3, 2, 4]
    srcs = [K.source(N, seed=70 + i) for i, N in enumerate(lens)]
    u = K.draws(lens, K.MAX_NEW, seed=3010)
    calls = [{"open": [0, 1, 2, 3], "push": {0: 5 * S, 1: 1, 2: 1, 3: 1}, "flush": []},
             {"open": [], "push": {1: 2, 2: 1, 3: 3}, "flush": [0, 1, 2, 3]}]
    pool = new_pool(dec, case, streams=4, slots=2)
    sid, log = drive(pool, case, srcs, u, calls)       # the rounds equal the twin's (drive asserts it)
    _, ticks, _, rounds = log[0]
    assert [rd[0][0] for rd in rounds] == [2 * S, S, S, S] and all(x is not None for x in rounds[0]), "5 S ids enter a ring of 2 S: 2 S, then S behind the S held"
    assert all(rd[1] is None and rd[2] is None and rd[3] is None for rd in rounds[1:]), "the later rounds run with whoever is left"
    assert {t[4] for t in ticks} == {0, 1, 2, 3}, "windows ran in every round"
    verify(w, dec, case, pool, sid, srcs, u)


def test_sixty_four_slots_eighty_streams_twice_in_one_state():
    case = Q.CASES["many"]
    w, dec = decoder("uniform")
    srcs, u = Q.inputs("many")
    srcs, u = srcs[:80], u[:80]
    calls = [{"open": list(range(80)), "push": {i: len(s) for i, s in enumerate(srcs)}, "flush": list(range(80))}]
    pool = new_pool(dec, case, streams=80, slots=64)
    sid_a, log_a = drive(pool, case, srcs, u, calls)
    assert pool.open_streams == 0
    sid_b, log_b = drive(pool, case, srcs, u, calls)
    assert min(sid_b.values()) == 80, "ids are never reused"
    assert log_a[0][1] == log_b[0][1]
    for i in range(80):
        assert torch.equal(pool.ids_of(sid_a[i]), pool.ids_of(sid_b[i])) and torch.equal(pool.logits_of(sid_a[i]), pool.logits_of(sid_b[i]))
        assert pool.stream(sid_a[i]).finish == pool.stream(sid_b[i]).finish
    verify(w, dec, case, pool, sid_b, srcs, u, rows=list(range(0, 80, 10)))
    assert all(0 <= p[0] < 64 for p in pool.last_placement) and max(a + b for a, b, *_ in log_b[0][1]) == 64, "every one of the 64 rows had a token in some tick"


def test_state_size_and_refusals_before_any_launch():
    w, dec = decoder("uniform")
    case = Q.CASES["single"]
    S, H, r = case["S"], case["H"], K.r
    pool = new_pool(dec, case, streams=3, slots=2)
    # the state: the queue's at the pool's max_len and tick_tokens, plus per stream 2 S source ids and r (S - H) + 1 carry ids, nothing else
    fn = dec._fn("pool_state_bytes")
    sizes = [int(fn(dec.handle, n, 2, pool.max_len, pool.tick_tokens, S, H, r)) for n in (1, 2, 3, 64, 65)]
    assert pool.state_bytes == sizes[2] and pool.max_len == pool_max_len(S, H, r, case["block"], case["max_new"])
    queue = int(dec._fn("queue_state_bytes")(dec.handle, 2, pool.max_len, pool.tick_tokens))
    r256 = lambda nbytes: (nbytes + 255) // 256 * 256          # the carver rounds every array to 256 bytes
    assert sizes == [queue + r256(n * 2 * S * 4) + r256(n * (r * (S - H) + 1) * 4) for n in (1, 2, 3, 64, 65)], "nothing else is kept per stream"
    for kw in (dict(streams=0), dict(streams=1025), dict(slots=0), dict(slots=65), dict(window=7), dict(max_new_tokens=0), dict(tick_tokens=2 + pool.max_len - 1)):
        with pytest.raises(ValueError):
            dec.stream_pool(**{**dict(streams=3, slots=2, window=S, hop=H, max_new_tokens=case["max_new"]), **kw})
    srcs, u = Q.inputs("single")
    a, b, c = pool.open(uniforms=u[6]), pool.open(uniforms=u[5][:3]), pool.open(uniforms=u[3])
    with pytest.raises(ValueError, match="all 3"):
        pool.open()
    pool.push({a: srcs[6][:5], c: srcs[3][:2]})
    calls, ticks, state = pool.calls, pool.last_ticks, pool._state.clone()
    ids_in = lambda: [pool.stream(s).ids_in for s in (a, b, c)]
    assert ids_in() == [5, 0, 2]
    bad = [(dict(items={99: [1]}), "unknown"), (dict(items={}, flush=[b]), "nothing pushed"), (dict(items={a: [1], b: [K.CFG.SEMANTIC_VOCAB_SIZE]}), "semantic ids"),
           (dict(items={a: [1], c: [-1]}), "semantic ids"), (dict(items={a: [0.5]}), "integers"), (dict(items={a: np.zeros(65536 - 4, dtype=np.int64)}), "at most"),
           (dict(items={a: srcs[6][5:], b: srcs[5]}, flush=[a, b]), "uniforms"), (dict(items={a: [1]}, flush=[c, c]), "twice")]
    for kw, match in bad:
        with pytest.raises(ValueError, match=match):
            pool.push(**kw)
        assert pool.calls == calls and ids_in() == [5, 0, 2] and pool.last_ticks == ticks, "a refused call reaches neither the library nor any stream"
    assert torch.equal(pool._state, state)
    pool.close(b)
    with pytest.raises(ValueError, match="closed"):
        pool.push({b: [1]})
    d = pool.open(uniforms=u[5])
    assert d == 3 and pool.stream(d).place == pool.stream(b).place, "a closed stream frees its place; its id is not reused"
    pool.push({a: srcs[6][5:], d: srcs[5], c: srcs[3][2:]}, flush=[a, d, c])
    with pytest.raises(ValueError, match="flushed"):
        pool.push({a: [1]})
    # the streams that shared the refused calls are what they would have been without them
    for s, i in ((a, 6), (d, 5), (c, 3)):
        alone = dec.to_acoustic_long([srcs[i]], window=S, hop=H, max_new_tokens=case["max_new"], temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u[i:i + 1])
        assert pool.stream(s).windows == alone.windows[0] and pool.stream(s).finish == alone.finish[0]
    verify(w, dec, case, pool, {6: a, 5: d, 3: c}, srcs, u, rows=[6, 5, 3])
    # the library's own refusals leave the host record as it was
    import ctypes as C
    pos = (C.c_int64 * 6)(*pool._pos)
    rc = dec._fn("pool_push")(dec.handle, pool._state.data_ptr(), pool._state.numel(), 3, 2, pool.max_len, pool.tick_tokens, pool._pos, 2, (C.c_int32 * 2)(0, 0),
                              None, (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 0), S, H, r, K.CFG.SEMANTIC_OFFSET, K.CFG.SEMANTIC_VOCAB_SIZE, K.CFG.INFER_TOKEN,
                              K.CFG.ACOUSTIC_OFFSET, K.CFG.codebook_size, K.CFG.STOP_TOKEN, case["max_new"], 0.8, 100, pool._status.data_ptr(), 1, (C.c_int64 * 2)(0, 0),
                              pool._status.data_ptr(), 2, pool._status.data_ptr(), pool._status.data_ptr(), None, None, None, 0, None, None, None, None, None)
    assert rc != 0 and list(pool._pos) == list(pos), "a place named twice"


# ---- all three stages ------------------------------------------------------------------------------------------------------------------------------------
# tests/test_semantic_stream_gpu.py's fixture, built anew: a 2-layer GPT at block 1024, the fine model at block 128, S = 8, H = 4. A pool has ONE
# max_new_tokens, so the lengths are that file's CASES' at 16: with finish == "max_new_tokens" a stream of k non-final windows has 12 k + 28 ids, which makes
# "exact_b"'s 84 ids T = 128 = W (what "exact_a" is at its own max_new_tokens of 4); covers_every_fine_schedule asserts the cover in both tests that use them.
from audiotoken_amd import AudioToken, Tokenizers  # noqa: E402
from audiotoken_amd import weights as W  # noqa: E402
from audiotoken_amd.configs import Wav2VecBertDecoderConfig  # noqa: E402
from audiotoken_amd.fine_decoder import fine_windows  # noqa: E402
from audiotoken_amd.fine_decoder import seeded_uniforms as fine_draws  # noqa: E402
from audiotoken_amd.semantic_decoder import acoustic_windows, coarse_codes, seeded_uniforms  # noqa: E402
from audiotoken_amd.semantic_pool import fine_pool_passes  # noqa: E402
from audiotoken_amd.semantic_stream import stream_schedule  # noqa: E402

from tests import fine_cases  # noqa: E402
from tests.test_semantic_stream_gpu import CASES as STREAM_CASES  # noqa: E402

WF, MAX_NEW = 128, 16
LENGTHS = {name: STREAM_CASES[name][0] for name in ("single", "short", "exact_b", "mid", "long")}
SIX = ["single", "short", "exact_b", "mid", "long", "long"]
SEEDS = [11, 12, 13, 14, 15, 16]


@pytest.fixture(scope="module")
def sem():
    gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    return AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))


def source(N, i=0):
    return (np.arange(N) * 7 + N + 3 * i) % 1000


def covers_every_fine_schedule(Ts):
    """Asserted, so that the lengths cannot silently degenerate: among the produced T one below W, one with (T - W) % H == 0, one past 2 W whose last window
    has rel > 0, one between W and 2 W with rel > 0; and every stream can be decoded (the acoustic decoder needs 7 frames)."""
    Hf = WF // 2
    assert any(T < WF for T in Ts) and any(T >= WF and (T - WF) % Hf == 0 for T in Ts)
    assert any(T > 2 * WF and (T - WF) % Hf != 0 for T in Ts) and any(WF < T < 2 * WF and (T - WF) % Hf != 0 for T in Ts)
    assert all(T >= 7 for T in Ts)


def audio_pool(sem, **kw):
    return sem.audio_stream_pool(**{**dict(window=8, hop=4, max_new_tokens=MAX_NEW, keep_codes=True), **kw})


def drive_audio(pool, srcs, calls, open_kw):
    """Run ``calls`` on the pool: per call ``{stream index: audio}``."""
    sid, at, outs = {}, [0] * len(srcs), []
    for c in calls:
        for i in c["open"]:
            sid[i] = pool.open(**open_kw[i])
        items = {}
        for i, m in c["push"].items():
            items[sid[i]] = srcs[i][at[i]:at[i] + m]
            at[i] += m
        got = pool.push(items, flush=[sid[i] for i in c["flush"]])
        named = sorted(set(c["push"]) | set(c["flush"]))
        assert sorted(got) == [sid[i] for i in named]
        assert all(a.dtype == torch.float32 and a.dim() == 2 and a.shape[0] == 1 and a.shape[1] % 320 == 0 and a.device.type == "cpu" for a in got.values())
        outs.append({i: got[sid[i]] for i in named})
    return sid, outs


def test_one_slot_one_fine_slot_is_audio_stream_piece_for_piece(sem):
    names = list(LENGTHS)
    srcs = [source(LENGTHS[n], i) for i, n in enumerate(names)]
    calls = P.interleaving([len(s) for s in srcs], 21, most=48, late=(4,), width=(2, 5))
    pool = audio_pool(sem, streams=5, slots=1, fine_slots=1)
    sid, outs = drive_audio(pool, srcs, calls, [dict(seed=SEEDS[i]) for i in range(5)])
    Ts = []
    for i, src in enumerate(srcs):
        solo = sem.audio_stream(window=8, hop=4, max_new_tokens=MAX_NEW, seed=SEEDS[i], keep_codes=True)
        at = 0
        for c, out in zip(calls, outs):
            if i not in out:
                continue
            want = []
            if i in c["push"]:
                want.append(solo.push(src[at:at + c["push"][i]]))
                at += c["push"][i]
            if i in c["flush"]:
                want.append(solo.flush())
            assert torch.equal(out[i], torch.cat(want, dim=-1)), f"stream {i}: the audio of every call"
        rec = pool.stream(sid[i])
        assert torch.equal(rec.coarse_ids, solo.coarse_ids) and torch.equal(rec.fine_codes, solo.fine_codes)
        assert rec.finish == solo.finish and rec.windows == solo.windows and rec.fine_windows_run == solo.fine_windows_run
        assert (rec.ids_in, rec.frames_in, rec.frames_out) == (solo.ids_in, solo.frames_in, solo.frames_out)
        Ts.append(rec.frames_in)
    print("frames per stream:", dict(zip(names, Ts)))
    covers_every_fine_schedule(Ts)


def test_four_slots_three_fine_slots_six_streams_interleaved(sem):
    srcs = [source(LENGTHS[n], i) for i, n in enumerate(SIX)]
    calls = P.interleaving([len(s) for s in srcs], 22, most=48, late=(5,), width=(3, 6))
    # explicit draws: what seed s gives (tests/test_semantic_stream_cpu.py pins the prefix rule), two spare fine windows
    us = [seeded_uniforms(SEEDS[i], 1, 3 * (len(s) + 8) + MAX_NEW + 64)[0] for i, s in enumerate(srcs)]
    fus = [fine_draws(SEEDS[i], 1, 3 * len(s) // WF + 4, WF)[0] for i, s in enumerate(srcs)]
    pool = audio_pool(sem, streams=6, slots=4, fine_slots=3)
    sizes = pool.state_bytes
    passes = []
    sid, at, outs, pieces = {}, [0] * 6, [], []
    ref = sem._fine_audio().decode_stream_pool(slots=6)
    ref_sid = {}
    for c in calls:
        for i in c["open"]:
            sid[i] = pool.open(uniforms=us[i], fine_uniforms=fus[i])
            ref_sid[i] = ref.open()
        items = {}
        for i, m in c["push"].items():
            items[sid[i]] = srcs[i][at[i]:at[i] + m]
            at[i] += m
        before = {i: pool.stream(sid[i]).fine_codes.shape[1] for i in sid}
        got = pool.push(items, flush=[sid[i] for i in c["flush"]])
        passes += pool.last_fine_passes
        named = sorted(set(c["push"]) | set(c["flush"]))
        outs.append({i: got[sid[i]] for i in named})
        # a fresh decode pool, pushed the same pieces in the same calls, returns the same tensors bit for bit
        new = {i: pool.stream(sid[i]).fine_codes[:, before[i]:] for i in named}
        want = {i: [] for i in named}
        fed = {ref_sid[i]: new[i].to(DEV) for i in named if new[i].shape[1]}
        if fed:
            for d, a in ref.push(fed).items():
                want[next(i for i in named if ref_sid[i] == d)].append(a)
        if c["flush"]:
            for d, a in ref.flush([ref_sid[i] for i in c["flush"]]).items():
                want[next(i for i in named if ref_sid[i] == d)].append(a)
        for i in named:
            w = torch.cat([a.reshape(1, -1) for a in want[i]], dim=-1).cpu() if want[i] else torch.empty((1, 0))
            assert torch.equal(got[sid[i]], w), f"stream {i}: the audio is the decode pool's"
    assert pool.state_bytes == sizes, "the state does not grow with the sources"
    covers_every_fine_schedule([pool.stream(sid[i]).frames_in for i in range(6)])
    assert any(n >= 2 for _, _, n in passes), "a fine pass held windows of at least two streams"
    for i, src in enumerate(srcs):
        rec = pool.stream(sid[i])
        N, T = len(src), rec.frames_in
        plan = acoustic_windows(N, 8, 4, 3, 1024)
        assert rec.windows[:-1] == plan[:-1] and rec.windows[-1][:3] == plan[-1][:3] and rec.ids_in == N
        assert rec.fine_windows_run == fine_windows(T, WF)
        codes = coarse_codes(rec.coarse_ids, sem._gpt().config.codebook_size, 2)
        assert codes.shape[1] == T
        n_win = len(fine_windows(T, WF))
        fine = sem.to_fine([codes], uniforms=fus[i][None, :n_win])
        assert torch.equal(rec.fine_codes, fine.codes[0]), f"stream {i}: the fine codes are to_fine's on its coarse codes with its draws"
        pushes = P.pushes_of(calls, i)
        merged = pushes[-1] != 0
        events = stream_schedule(pushes if merged else pushes[:-1], 8, 4, 3, 1024, WF, final_budget_result=rec.windows[-1][3], max_new_tokens=MAX_NEW)
        emitted = [0 if e["emit"] is None else e["emit"][1] - e["emit"][0] for e in events]
        if merged:
            emitted = emitted[:-2] + [emitted[-2] + emitted[-1]]
        mine = [out[i].shape[-1] // 320 for out in outs if i in out]
        assert mine == emitted and sum(mine) == T == rec.frames_out, "frames leave in the call in which they turn final"
    # the state sizes are the size queries' values: per stream 2 S + r (S - H) + 1 ints of GPT state and 2 W * 8 ints of fine state
    gpt, fine = sem._gpt(), sem._fine()
    gp = pool.gpt_pool
    g = lambda n: int(gpt._fn("pool_state_bytes")(gpt.handle, n, 4, gp.max_len, gp.tick_tokens, 8, 4, 3))
    f = lambda n: int(fine._fn("pool_state_bytes")(fine.handle, n, 3))
    assert sizes == (g(6), f(6))
    assert g(64 + 6) - g(6) == 64 * 4 * (2 * 8 + 3 * 4 + 1) and f(7) - f(6) == 2 * WF * 8 * 4


def test_audio_pool_refusals(sem):
    pool = audio_pool(sem, streams=2, slots=1, fine_slots=1)
    with pytest.raises(ValueError, match="voice"):
        sem.audio_stream_pool(voice=object())
    for kw in (dict(streams=0), dict(streams=1025), dict(slots=65), dict(fine_slots=0), dict(fine_slots=65), dict(window=7), dict(max_new_tokens=0), dict(top_p=0.0)):
        with pytest.raises(ValueError):
            audio_pool(sem, **{**dict(streams=2, slots=1, fine_slots=1), **kw})
    fu = fine_draws(5, 1, 1, WF)[0]
    a = pool.open(seed=1)
    b = pool.open(seed=2, fine_uniforms=fu)            # one window's draws: runs out at the second fine window
    with pytest.raises(ValueError, match="all 2"):
        pool.open()
    src = source(176)
    pool.push({a: src[:20], b: src[:20]})
    calls = pool.gpt_pool.calls
    state = lambda: [(pool.stream(s).ids_in, pool.stream(s).frames_in, pool.stream(s).frames_out) for s in (a, b)]
    was = state()
    for kw, match in [(dict(items={7: [1]}), "unknown"), (dict(items={a: [1000000]}), "semantic ids"), (dict(items={a: src[20:40], b: src[20:]}), "fine_uniforms"),
                      (dict(items={a: [1]}, flush=[a, a]), "twice")]:
        with pytest.raises(ValueError, match=match):
            pool.push(**kw)
        assert pool.gpt_pool.calls == calls and state() == was, "a refused call leaves every stream as it was"
    # a stream refused for its draws does not disturb the other: a, pushed on alone, is audio_stream(seed=1)
    pool.close(b)
    c = pool.open(seed=3)
    assert c == 2
    got = [pool.push({a: src[20:]})[a], pool.push({c: [5]}, flush=[a])]
    solo = sem.audio_stream(window=8, hop=4, max_new_tokens=MAX_NEW, seed=1, keep_codes=True)
    want = [solo.push(src[:20]), solo.push(src[20:]), solo.flush()]
    assert torch.equal(got[0], want[1]) and torch.equal(got[1][a], want[2]) and torch.equal(pool.stream(a).fine_codes, solo.fine_codes)
    assert pool.stream(a).state == "flushed" and pool.stream(a).finish == solo.finish


def test_a_stream_with_no_whole_frame_raises_at_its_flush_and_leaves_the_others_alone():
    """The STOP row of ``wte`` scaled by 30 (tests/gpt_queue_cases.py's trick on this vocabulary): the one-id source [5] draws STOP at step 0 whatever its draw
    (its logit leads by about 100), so its stream has no frame; the 13-id stream beside it has its two non-final windows' 18 frames, which cannot stop."""
    cfg = Wav2VecBertDecoderConfig()
    gpt = W.synth_gpt_weights(n_layer=2, vocab=cfg.VOCAB_SIZE, block=1024, seed=0, family="peaky")
    wte = gpt["transformer.wte.weight"].copy()
    wte[cfg.STOP_TOKEN] *= 30.0
    stop = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights={**gpt, "transformer.wte.weight": wte}, fine_weights=fine_cases.weights("a", "peaky"))
    pool = audio_pool(stop, streams=2, slots=1, fine_slots=1)   # one row: b's ticks are the solo stream's, so the comparison below is exact
    a, b = pool.open(seed=1), pool.open(seed=2)
    src = source(13)
    with pytest.raises(ValueError, match="produced no whole frame"):
        pool.push({a: [5], b: src}, flush=[a, b])
    assert pool.stream(a).state == "flushed" and pool.stream(a).finish == "stop" and pool.stream(a).frames_in == 0
    solo = stop.audio_stream(window=8, hop=4, max_new_tokens=MAX_NEW, seed=2, keep_codes=True)
    want = torch.cat([solo.push(src), solo.flush()], dim=-1)
    rec = pool.stream(b)
    assert rec.state == "flushed" and rec.windows == solo.windows and rec.finish == solo.finish and rec.frames_out == solo.frames_out >= 18
    assert torch.equal(rec.fine_codes, solo.fine_codes) and torch.equal(pool.last_output[b], want)
    c = pool.open(seed=3)
    assert c == 2 and pool.gpt_pool.open_streams == 1, "both places are free again"


def test_a_flushed_stream_whose_fine_draws_are_short_is_refused_before_any_launch_and_the_others_go_on(sem):
    """A flushed stream's length is the device's to decide, so its explicit ``fine_uniforms`` must cover the longest it can get. One window's draws for a
    stream that will have three: the call that flushes it is refused whole, before stage 1 runs; the two streams beside it in that call are untouched and,
    pushed on, equal their solo streams piece for piece."""
    pool = audio_pool(sem, streams=3, slots=1, fine_slots=1)
    src = [source(176, 0), source(130, 1), source(84, 2)]
    a = pool.open(seed=31, fine_uniforms=fine_draws(31, 1, 1, WF)[0])
    b, c = pool.open(seed=32), pool.open(seed=33)
    solo = {s: sem.audio_stream(window=8, hop=4, max_new_tokens=MAX_NEW, seed=seed, keep_codes=True) for s, seed in ((b, 32), (c, 33))}
    first = pool.push({a: src[0][:60], b: src[1][:50], c: src[2][:40]})          # a: 13 non-final windows, 84 frames, no fine window yet
    assert torch.equal(first[b], solo[b].push(src[1][:50])) and torch.equal(first[c], solo[c].push(src[2][:40]))
    state = lambda: [(pool.stream(s).ids_in, pool.stream(s).frames_in, pool.stream(s).frames_out, len(pool.stream(s).windows)) for s in (a, b, c)]
    was, calls, gpt_state, fine_state = state(), pool.gpt_pool.calls, pool.gpt_pool._state.clone(), pool._fine_state.clone()
    with pytest.raises(ValueError, match="fine_uniforms"):
        pool.push({a: src[0][60:], b: src[1][50:90], c: src[2][40:]}, flush=[a, c])
    assert pool.gpt_pool.calls == calls and state() == was and pool.stream(a).state == "open", "refused before stage 1: no stream of the call moved"
    assert torch.equal(pool.gpt_pool._state, gpt_state) and torch.equal(pool._fine_state, fine_state)
    got = pool.push({b: src[1][50:90], c: src[2][40:]}, flush=[c])
    assert torch.equal(got[b], solo[b].push(src[1][50:90])) and torch.equal(got[c], torch.cat([solo[c].push(src[2][40:]), solo[c].flush()], dim=-1))
    got = pool.push({b: src[1][90:]}, flush=[b])
    assert torch.equal(got[b], torch.cat([solo[b].push(src[1][90:]), solo[b].flush()], dim=-1))
    for s in (b, c):
        rec = pool.stream(s)
        assert torch.equal(rec.coarse_ids, solo[s].coarse_ids) and torch.equal(rec.fine_codes, solo[s].fine_codes) and rec.finish == solo[s].finish
        assert rec.windows == solo[s].windows and rec.fine_windows_run == solo[s].fine_windows_run
    pool.close(a)
