"""CPU: the generation queue without a device: the scheduler's invariants over a sweep of lengths, slots, ``tick_tokens`` and simulated stop
steps; the same cases through the library's own scheduler (tools/gpt_queue_args.hip, a stand-alone program under the host sanitizers), whose printed ticks
must equal the Python twin's; its refusal paths; what the twin alone says about the GPU file's inputs (tests/gpt_queue_cases.py: few draws near a CDF
boundary); and the interface's refusals that need no device."""
import os
import subprocess

import numpy as np
import pytest

from audiotoken_amd import AudioToken, Tokenizers, _cabi
from audiotoken_amd.semantic_decoder import (CHECK_EVERY, AcousticGeneration, acoustic_windows, queue_tick_bound, queue_ticks, window_steps)

from tests import gpt_queue_cases as Q
from tests import long_form_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (S, H, block, max_new, lengths): the small geometry, the two-route geometry and the product geometry
GEOMETRIES = [
    (8, 4, 64, 10, [1, 7, 8, 9, 12, 13, 19] * 3),
    (16, 8, 128, 10, Q.CASES["routes"]["lens"]),
    (250, 124, 1024, 64, [375, 251, 30, 1500, 100, 626]),
]


def sweep():
    for S, H, block, max_new, lens in GEOMETRIES:
        plans = [window_steps(acoustic_windows(N, S, H, 3, block), max_new, block) for N in lens]
        max_len = max(P + n for plan in plans for P, n in plan)
        budgets = [plan[-1][1] for plan in plans]
        for slots in (1, 3, 8, 64):
            for c in (1, 2, 8):
                for ends in ("budget", "one", "spread"):
                    e = {"budget": budgets, "one": [1] * len(lens), "spread": [1 + (5 * i) % b for i, b in enumerate(budgets)]}[ends]
                    yield S, H, block, max_new, lens, slots, slots + c * max_len, e, plans


def test_scheduler_invariants():
    n_cases = 0
    for S, H, block, max_new, lens, slots, tick_tokens, ends, plans in sweep():
        ticks, placement, events = queue_ticks(lens, S, H, 3, block, max_new, slots, tick_tokens, ends, detail=True)
        n_cases += 1
        assert len(ticks) == len(events) <= queue_tick_bound(lens, S, H, 3, block, max_new), "termination within the stated bound"
        ran = [[] for _ in lens]          # per source: (window, tick of its prefill)
        sampled = {}                      # (source, window) -> sampler launches
        holder = {}                       # slot -> source
        final_start = {}
        for at, ((a, b, c, route), (steps, starts, poll, waiting)) in enumerate(zip(ticks, events)):
            assert (a, b, c) == (len(steps), len(starts), sum(x[3] for x in starts)) and route == (1 if a + c > 64 else 0)
            assert 1 <= a + c <= tick_tokens, "no tick exceeds tick_tokens or is empty"
            slots_in_tick = [x[0] for x in steps] + [x[0] for x in starts]
            assert len(set(slots_in_tick)) == len(slots_in_tick), "a slot has one token run per tick: it never steps in the tick it prefills"
            assert not set(waiting) & set(slots_in_tick) and (not waiting or starts or a > 0)
            if waiting:
                first = min(waiting)
                assert all(x[0] < first for x in starts), "admission goes in slot order and stops at the first window that does not fit"
                here = [s for s in range(len(lens)) if placement[s][0] == first and placement[s][2] >= at]   # in the slot now, or the next to begin in it
                src = min(here, key=lambda s: placement[s][1])
                assert a + c + plans[src][len(ran[src])][0] > tick_tokens, "a window waits only because it does not fit"
            for j, src, k, P in starts:
                assert P == plans[src][k][0]
                assert k == len(ran[src]), "every source runs its windows in order and exactly once"
                ran[src].append((k, at))
                if k == 0:
                    assert placement[src][:2] == (j, at)
                    assert j not in holder or placement[holder[j]][2] < at, "a slot never holds two sources"
                    holder[j] = src
                assert holder[j] == src
                sampled[(src, k)] = 1
                if k == len(plans[src]) - 1:
                    final_start[src] = at
            for j, src, k in steps:
                assert holder[j] == src and (src, k) in sampled and k == len(ran[src]) - 1, "a slot steps only after its prefill, in its current window"
                assert at <= placement[src][2]
                sampled[(src, k)] += 1
            if poll:
                assert (at + 1) % CHECK_EVERY == 0
        slack = 0
        for src, plan in enumerate(plans):
            assert [k for k, _ in ran[src]] == list(range(len(plan)))
            for k, (P, n) in enumerate(plan[:-1]):
                assert sampled[(src, k)] == n, "a non-final window samples its exact count"
            e = min(ends[src], plan[-1][1])
            done_at = final_start[src] + e - 1          # the tick of the final window's last needed sample
            last = placement[src][2]
            assert done_at <= last < done_at + CHECK_EVERY and sampled[(src, len(plan) - 1)] == last - final_start[src] + 1
            poll_at = done_at + (-(done_at + 1)) % CHECK_EVERY           # the first tick from done_at on that ends with a poll
            budget_at = final_start[src] + plan[-1][1] - 1               # the tick of the budget's last sample, which the host knows
            assert last == min(poll_at, budget_at), "an early end is seen at the next poll, a used-up budget at once"
            slack += last - done_at
        needed = sum(n - 1 for plan in plans for _, n in plan[:-1]) + sum(min(ends[i], plan[-1][1]) - 1 for i, plan in enumerate(plans))
        assert sum(t[0] for t in ticks) == needed + slack, "step tokens: what the windows need plus the slack before polls"
        assert sum(t[1] for t in ticks) == sum(len(plan) for plan in plans)
    assert n_cases == 3 * 4 * 3 * 3


def test_scheduler_refusals_and_defaults():
    for kw in (dict(slots=0), dict(slots=65), dict(tick_tokens=4 + 20), dict(lens=[])):   # the longest prompt has 21 tokens
        args = {**dict(lens=[19, 1], slots=4, tick_tokens=4 + 33), **kw}
        with pytest.raises(ValueError):
            queue_ticks(args["lens"], 8, 4, 3, 64, 10, args["slots"], args["tick_tokens"])
    with pytest.raises(ValueError):
        queue_ticks([1] * 4097, 8, 4, 3, 64, 10, 4, 100)
    ticks, placement = queue_ticks([19, 1], 8, 4, 3, 64, 10, 4, 4 + 33)
    assert ticks[0] == (0, 2, 11, 0) and placement[1] == (1, 0, 9)
    assert AcousticGeneration(ids=[], codes=[], finish=[]).ticks is None and AcousticGeneration(ids=[], codes=[], finish=[]).placement is None


def run_tool(args=""):
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "gpt_queue_asan"] + (["QUEUE_ARGS=" + args] if args else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
    return out.stdout


def test_argument_checks_under_the_sanitizers():
    assert "gpt queue argument checks: ok" in run_tool()


def test_the_librarys_scheduler_equals_the_twin():
    """The same sweep through ``GptQueueSchedule`` (csrc/gpt.h), dry-run by the stand-alone program: its ticks and placement must equal ``queue_ticks``'."""
    run_tool()   # builds it once
    exe = os.path.join(ROOT, "audiotoken_amd", "csrc", "build_asan", "gpt_queue_args")
    n_cases = 0
    for S, H, block, max_new, lens, slots, tick_tokens, ends, _ in sweep():
        if slots == 3 and tick_tokens % 2:      # a third of the sweep is enough here: every geometry, slot count and end rule still occurs
            continue
        out = subprocess.run([exe, "dry"] + [str(x) for x in (S, H, 3, block, max_new, slots, tick_tokens)] + [f"{N}:{e}" for N, e in zip(lens, ends)],
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
        lines = out.stdout.split("\n")
        got_ticks = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("tick ")]
        got_place = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("source ")]
        ticks, placement = queue_ticks(lens, S, H, 3, block, max_new, slots, tick_tokens, ends)
        assert got_ticks == ticks and got_place == placement, (S, H, slots, tick_tokens)
        n_cases += 1
    assert n_cases >= 60
    bad = subprocess.run([exe, "dry", "8", "4", "3", "64", "10", "4", "24", "19:1"], capture_output=True, text=True, timeout=120)
    assert bad.returncode == 2 and "refused" in bad.stdout


@pytest.mark.parametrize("case", sorted(Q.CASES))
def test_the_twins_own_chain_rarely_meets_a_boundary(case):
    """The GPU protocol may waive an id where the draw lies within 2 (kept 2^-24 + 2^-22) of a CDF boundary, for at most 2 % of a test's steps. On the
    twin's own chain, for exactly the sources, draws and weights of every GPU case, the share of such draws stays under that cap (the product geometry is
    left out as in tests/test_long_form_cpu.py: its uncached steps over contexts of 1000 ids would take minutes on a CPU)."""
    c = Q.CASES[case]
    srcs, u = Q.inputs(case)
    for family in c["families"]:
        w = Q.weights(family, c["block"])
        inside = steps = 0
        empty_finals = 0
        for i, src in enumerate(srcs):
            stream, finish, trace = K.twin_chain(w, K.CFG, src, u[i], max_new=c["max_new"], S=c["S"], H=c["H"], block=c["block"])
            plan = acoustic_windows(len(src), c["S"], c["H"], K.r, c["block"])
            empty_finals += finish == "stop" and len(stream) == K.r * plan[-1][0] + plan[-1][2]
            for _, dist, kept in trace:
                steps += 1
                inside += dist < 2.0 * (kept * 2.0 ** -24 + 2.0 ** -22)
        print(f"{case} / {family}: {inside} of {steps} draws inside the window; {empty_finals} final windows stop at once")
        assert inside <= 0.02 * steps
        if case == "stop":
            assert empty_finals >= 1, "the STOP-heavy case has a source with no ids in its final window"


def test_interface_refusals():
    for tok in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        for kw in (dict(slots=4), dict(tick_tokens=100), dict(slots=4, window=8, hop=4)):
            with pytest.raises(ValueError, match="long_form"):
                AudioToken(tok, device="cuda:0").to_acoustic(np.arange(4), **kw)
            with pytest.raises(ValueError, match="long_form"):
                AudioToken(tok, device="cuda:0").to_audio(np.arange(4), **kw)
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_acoustic(np.arange(4), long_form=True, slots=4)
    with pytest.raises(ValueError, match="semantic"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_audio(np.arange(4), long_form=True, slots=4)
    lib = _cabi.load()
    assert lib.at_gpt_queue_state_bytes(None, 4, 33, 37) == 0 and "not finalized" in _cabi.last_error()
