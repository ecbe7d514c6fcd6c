"""CPU: the rule of one stream pool call: ``pool_schedule`` against a brute-force restatement (independent §25 streams merged tick by
tick, tests/semantic_pool_cases.py), every stream's windows against ``stream_schedule`` of its own pushes, and the library's ``GptPoolSchedule`` and its
refusal paths through the stand-alone program under the host sanitizers (``make audio_stream_pool_asan``)."""
import os
import subprocess

import numpy as np
import pytest

from audiotoken_amd.semantic_decoder import acoustic_windows
from audiotoken_amd.semantic_pool import fine_pool_passes, pool_max_len, pool_schedule
from audiotoken_amd.fine_decoder import fine_windows
from audiotoken_amd.semantic_stream import stream_schedule

from tests import semantic_pool_cases as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S, H, r, BLOCK, MAX_NEW, W = 8, 4, 3, 64, 10, 16
MAX_LEN = pool_max_len(S, H, r, BLOCK, MAX_NEW)


def sweep():
    rng = np.random.default_rng(11)
    for seed in range(6):
        lens = rng.integers(1, 5 * S, size=int(rng.integers(1, 9))).tolist()
        if seed == 0:
            lens[0] = 5 * S + 3                  # a push that takes several rounds
        calls = P.interleaving(lens, seed, most=(5 * S + 3 if seed == 0 else 6), late=(len(lens) - 1,) if len(lens) > 1 else (), width=(1, 8))
        for slots in (1, 2, 4, len(lens) + 3):
            for tick_tokens in (slots + MAX_LEN, slots + 2 * MAX_LEN):
                yield lens, calls, slots, tick_tokens, rng


def test_pool_schedule_is_the_brute_force_merge_and_every_stream_its_own_schedule():
    n_cases = 0
    for lens, calls, slots, tick_tokens, rng in sweep():
        windows = [[] for _ in lens]
        per_call = [[] for _ in lens]
        for streams in P.call_streams(calls, len(lens)):
            if not streams:
                continue
            arg = [(b, m, f) for _, b, m, f in streams]
            # final windows that end early, so that polls matter
            ends = [int(rng.integers(1, MAX_NEW + 2)) for _ in arg]
            rounds, ticks, placement, events = pool_schedule(arg, S, H, r, BLOCK, MAX_NEW, slots, tick_tokens, final_steps=ends, detail=True)
            brute, ran = P.brute_call(arg, S, H, r, BLOCK, MAX_NEW, slots, tick_tokens, final_steps=ends)
            assert len(ticks) == len(brute)
            for (a, b, c, route, g), (steps, starts, polled, waiting), (bg, tick) in zip(ticks, events, brute):
                mine = [(j, i, k, 1) for j, i, k in steps] + [(j, i, k, Pn) for j, i, k, Pn, _ in starts]
                assert mine == [(j, i, k, t) for j, i, k, _, t in tick] and g == bg
                assert 1 <= a + c <= tick_tokens and (a, b) == (len(steps), len(starts)) and route == (1 if a + c > 64 else 0)
            assert len(rounds) == (max(t[4] for t in ticks) + 1 if ticks else len(rounds))
            for x, (i, b, m, f) in enumerate(streams):
                windows[i] += ran[x]
                per_call[i].append(ran[x])
                # the ring: what is held and taken in a round never exceeds 2 S
                assert all(rd[x] is None or rd[x][0] + rd[x][1] <= 2 * S for rd in rounds)
                started = [(k, fin) for _, starts, _, _ in events for _, s, k, _, fin in starts if s == x]
                assert started == ran[x], "a stream's windows start in order, each once"
                assert (placement[x][1] >= 0) == bool(ran[x])
            n_cases += 1
        for i, N in enumerate(lens):
            plan = acoustic_windows(N, S, H, r, BLOCK)
            assert windows[i] == [(k, k == len(plan) - 1) for k in range(len(plan))], "the union of a stream's calls is acoustic_windows(N)"
            pushes = P.pushes_of(calls, i)
            events = stream_schedule(pushes[:-1] if pushes[-1] == 0 else pushes, S, H, r, BLOCK, W, max_new_tokens=MAX_NEW)
            mine = [c for c in per_call[i]]
            if pushes[-1] != 0:                  # pushed and flushed in one call: §25's push and flush events together
                want = [e["gpt"] for e in events[:-2]] + [events[-2]["gpt"] + events[-1]["gpt"]]
            else:
                want = [e["gpt"] for e in events]
            assert mine == want, "every call's windows are stream_schedule's for that push"
    assert n_cases > 100


def test_pool_schedule_refuses():
    with pytest.raises(ValueError):
        pool_schedule([(0, 1, True)], S, H, r, BLOCK, MAX_NEW, 0, 100)
    with pytest.raises(ValueError):
        pool_schedule([(0, 1, True)], S, H, r, BLOCK, MAX_NEW, 2, 2 + MAX_LEN - 1)
    with pytest.raises(ValueError):
        pool_schedule([(0, 1, True)], 7, H, r, BLOCK, MAX_NEW, 2, 200)
    assert pool_schedule([(3, 0, False)], S, H, r, BLOCK, MAX_NEW, 2, 200) == ([], [], [(-1, -1, -1)])


def run_program(args):
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "audio_stream_pool_asan"] + (["POOL_ARGS=" + args] if args else [])
    done = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stdout[-3000:] + done.stderr[-3000:]
    assert "AddressSanitizer" not in done.stdout + done.stderr and "runtime error" not in done.stdout + done.stderr
    return done.stdout


def test_library_scheduler_equals_the_twin_and_refusals_hold_under_the_sanitizers():
    out = run_program("")
    assert "all refusals refused" in out and "0 launches" in out
    rng = np.random.default_rng(5)
    for slots, tick_tokens in ((1, 1 + MAX_LEN), (3, 3 + MAX_LEN), (4, 4 + 2 * MAX_LEN)):
        streams = [(int(rng.integers(0, 3 * S)), int(rng.integers(0, 5 * S)), bool(rng.integers(0, 2))) for _ in range(7)]
        streams = [(b, m, f and b + m > 0) for b, m, f in streams]
        ends = [int(rng.integers(1, MAX_NEW + 2)) for _ in streams]
        words = " ".join(f"{b}:{m}:{int(f)}:{e}" for (b, m, f), e in zip(streams, ends))
        out = run_program(f"gpt {S} {H} {r} {BLOCK} {MAX_NEW} {slots} {tick_tokens} {words}")
        rounds, ticks, placement = pool_schedule(streams, S, H, r, BLOCK, MAX_NEW, slots, tick_tokens, final_steps=ends)
        got_ticks = [tuple(int(v) for v in line.split()[1:]) for line in out.splitlines() if line.startswith("tick ")]
        got_rounds = [tuple(int(v) for v in line.split()[1:]) for line in out.splitlines() if line.startswith("round ")]
        got_place = [tuple(int(v) for v in line.split()[1:]) for line in out.splitlines() if line.startswith("place ")]
        assert got_ticks == ticks and got_place == placement
        want_rounds = [(g, i) + tuple(x) for g, rd in enumerate(rounds) for i, x in enumerate(rd) if x is not None]
        assert got_rounds == want_rounds


def fine_calls(seed, n, Wf):
    """Random calls of a fine pool: per call ``[(stream, frames before, frames handed over, final)]``."""
    rng = np.random.default_rng(seed)
    total = rng.integers(1, 7 * Wf, size=n).tolist()
    had, done, calls = [0] * n, [False] * n, []
    while not all(done):
        call = []
        for i in range(n):
            if done[i] or rng.random() < 0.3:
                continue
            m = min(total[i] - had[i], int(rng.integers(0, 3 * Wf)))
            final = had[i] + m == total[i] and (m == 0 or rng.random() < 0.5)
            call.append((i, had[i], m, final))
            had[i] += m
            done[i] = final
        if call:
            calls.append(call)
    return total, calls


def test_fine_pool_passes_keep_every_stream_on_its_own_schedule():
    Wf = 16
    for seed in range(8):
        total, calls = fine_calls(seed, 1 + seed % 5, Wf)
        for fine_slots in (1, 2, 3, 9):
            ran = [[] for _ in total]
            for call in calls:
                rounds, passes = fine_pool_passes([(b, m, f) for _, b, m, f in call], Wf, fine_slots)
                for rd in rounds:
                    assert all(x is None or x[2] + x[0] + x[5] <= 2 * Wf for x in rd), "no fine cell array exceeds 2 W"
                last = (-1, -1)
                for g, wave, wins in passes:
                    assert 1 <= len(wins) <= fine_slots and len({i for i, _, _ in wins}) == len(wins), "two windows of one stream never share a pass"
                    assert (g, wave) >= last, "rounds in order, waves in order inside a round"
                    last = (g, wave)
                    for i, j, rel in wins:
                        ran[call[i][0]].append((j, rel))
            H = Wf // 2
            for i, T in enumerate(total):
                want = [(k, fill - start) for k, (start, fill) in enumerate(fine_windows(T, Wf))]
                assert ran[i] == want, "the union of a stream's calls is fine_windows(T, W), in order"


def test_library_fine_scheduler_equals_the_twin():
    Wf = 16
    for seed, fine_slots in ((1, 1), (2, 2), (3, 4)):
        _, calls = fine_calls(seed, 5, Wf)
        call = max(calls, key=len)
        words = " ".join(f"{b}:{m}:{int(f)}" for _, b, m, f in call)
        out = run_program(f"fine {Wf} {fine_slots} {words}")
        rounds, passes = fine_pool_passes([(b, m, f) for _, b, m, f in call], Wf, fine_slots)
        got_rounds = [tuple(int(v) for v in line.split()[1:]) for line in out.splitlines() if line.startswith("round ")]
        got_passes = [line.split()[1:] for line in out.splitlines() if line.startswith("pass ")]
        assert got_rounds == [(g, i) + tuple(int(v) for v in x) for g, rd in enumerate(rounds) for i, x in enumerate(rd) if x is not None]
        assert [(int(p[0]), int(p[1]), [tuple(int(v) for v in w.split(":")) for w in p[2:]]) for p in got_passes] == passes
