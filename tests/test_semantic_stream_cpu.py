"""CPU: the semantic-to-audio stream without a device: the rule's twin (``semantic_stream.stream_schedule``) against a brute-force
statement of it over every push splitting; the prefix property of both draws; the GPT and the fine twins chained under the stream's schedule against the
offline twins; and the library's host side (tools/semantic_stream_args.hip, a stand-alone program under the host sanitizers): its refusal paths, and
its two schedulers round for round against their Python twins."""
import os
import subprocess

import numpy as np
import pytest

from audiotoken_amd import fine_decoder, semantic_decoder
from audiotoken_amd.fine_decoder import fine_windows
from audiotoken_amd.semantic_decoder import acoustic_windows
from audiotoken_amd.semantic_stream import (_Draws, fine_capacity, fine_stream_rounds, fine_windows_run, gpt_stream_rounds, gpt_windows_run, stream_schedule)

from tests import fine_cases, fine_ref
from tests import long_form_cases as K
from tests import semantic_stream_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 3
GEOMETRIES = [(8, 4, 64), (16, 8, 128)]   # (S, H_g, block)
WINDOWS = [128, 256]
MAX_NEW = 10


def check_case(N, S, H_g, block, W, pushes, result, max_new=MAX_NEW):
    H = W // 2
    events = stream_schedule(pushes, S, H_g, R, block, W, final_budget_result=result, max_new_tokens=max_new)
    assert len(events) == len(pushes) + 1
    n_in = np.cumsum(list(pushes) + [0])
    plan = acoustic_windows(N, S, H_g, R, block)
    # ---- the GPT windows: acoustic_windows(N) exactly, each in the first push at which one id past it existed, the final one at the flush alone
    ran = [(k, f, i) for i, e in enumerate(events) for k, f in e["gpt"]]
    assert [k for k, _, _ in ran] == list(range(len(plan))) and [f for _, f, _ in ran] == [False] * (len(plan) - 1) + [True]
    assert events[-1]["gpt"] == [(len(plan) - 1, True)], "every non-final window has run by the time of the flush"
    for k, f, i in ran[:-1]:
        first = int(np.argmax(n_in > k * H_g + S))
        assert i == first and n_in[i] > k * H_g + S, "a window runs in the first push after which one id past it exists"
        assert all(n_in[q] <= k * H_g + S for q in range(i)), "and not at n_in == k H + S, where it might still be the final one"
    ids = 0
    for (start, n_src, carry, new), (k, f, i) in zip(plan, ran):
        assert start == k * H_g and ids == R * start + carry
        ids += new if new is not None else result
    # ---- the frames and the fine windows: fine_windows(T, W) exactly, each eager one in the first call at which its W frames existed
    T = ids // 2
    assert events[-1]["frames"] == T
    fine = [(w, i) for i, e in enumerate(events) for w in e["fine"]]
    if T == 0:
        assert not fine and all(e["emit"] is None for e in events)
        return T
    want = fine_windows(T, W)
    assert [w for w, _ in fine] == want
    frames = [e["frames"] for e in events]
    for j, ((start, fill), i) in enumerate(fine):
        if start == j * H and start + W <= T:
            assert i == int(np.argmax(np.asarray(frames) >= start + W)), "a fine window runs in the first call at which its frames exist"
        else:
            assert i == len(events) - 1, "only the flush runs a padded window or one at start = T - W"
    # ---- no frame is emitted before the last window that writes it; the frames are 0 .. T - 1, in order, once each
    last_writer = np.full(T, -1)
    for (w, i), frames_w in zip(fine, SC.write_sets([w for w, _ in fine], T, W)):
        last_writer[list(frames_w)] = i
    assert (last_writer >= 0).all(), "every frame is written by some window"
    at = 0
    for i, e in enumerate(events):
        assert e["held"] <= fine_capacity(W), "the window onto the row never exceeds its capacity"
        if e["emit"] is None:
            continue
        lo, hi = e["emit"]
        assert lo == at and hi > lo
        assert (last_writer[lo:hi] <= i).all(), "a frame goes out only after the last window that writes it"
        at = hi
    assert at == T
    return T


@pytest.mark.parametrize("S,H_g,block", GEOMETRIES)
@pytest.mark.parametrize("W", WINDOWS)
def test_the_twin_schedule_against_brute_force(S, H_g, block, W):
    n = 0
    for N in range(1, 3 * S + 6):
        for name, pushes in SC.splittings(N, S, H_g).items():
            for result in (MAX_NEW, 1, 0, 7):
                check_case(N, S, H_g, block, W, pushes, result)
                n += 1
    assert n == (3 * S + 5) * 5 * 4


def test_the_twin_schedule_on_sources_long_enough_for_every_fine_case():
    """The grid above never fills a fine window (3 S + 5 ids make fewer than W frames). These sources do: among their T are one below W, one with
    (T - W) % H == 0 and one past 2 W with a last window at rel > 0."""
    S, H_g, block, W = 8, 4, 64, 128
    seen = set()
    for N, result in ((20, 10), (44, 10), (86, 4), (130, 7), (176, 10)):
        for pushes in SC.splittings(N, S, H_g).values():
            T = check_case(N, S, H_g, block, W, pushes, result)
        seen.add("short" if T < W else "exact" if (T - W) % (W // 2) == 0 else "long" if T > 2 * W else "mid")
    assert seen == {"short", "exact", "long", "mid"}, seen


def test_fine_rounds_against_brute_force():
    """``fine_stream_rounds`` alone over every T up to 2 W + 70 in random splits: the windows are ``fine_windows(T, W)``, every round stays inside the
    window onto the row, a window's cells are held when it runs (the last one reads down to the start of the window before it), and a frame is emitted
    after the last window that writes it, within a round too."""
    for W in WINDOWS:
        H = W // 2
        rng = np.random.default_rng(W)
        for T in list(range(1, 2 * W + 71)) + [5 * W + 3]:
            for split in range(3):
                cuts = sorted(set(rng.integers(1, T, size=split * 3).tolist())) if T > 1 and split else []
                pieces = np.diff([0] + cuts + [T]).tolist() + [0]
                before, wins, emitted, first_held = 0, [], 0, 0
                for i, n_new in enumerate(pieces):
                    final = i == len(pieces) - 1
                    for take, first, held, j_first, n_win, pad, last, rel, e0, e1, shift in fine_stream_rounds(before, n_new, final, W):
                        assert first == first_held and 0 <= held and held + take + pad <= fine_capacity(W)
                        now = first + held + take
                        for j in range(j_first, j_first + n_win):
                            assert first <= j * H and (j * H + W <= now or pad), "the window's cells are in the array"
                            wins.append((j * H, j * H))
                        if last:
                            assert final and first <= now - W and 0 < rel <= H
                            wins.append((now - W, now - W + rel))
                        assert e0 == emitted and first <= e0 and e1 <= now
                        emitted = e1
                        first_held = first + shift
                    before += n_new
                assert wins == fine_windows(T, W) and emitted == T
                assert sum(1 for start, fill in wins if start == fill and start + W <= T) == fine_windows_run(T, W)


def test_gpt_rounds_never_overfill_the_source_buffer():
    for S, H_g, _ in GEOMETRIES + [(250, 124, 1024)]:
        for n_before in (0, 1, S, S + 1, 3 * S + 2):
            for n_new in (0, 1, S, 2 * S + 1, 7 * S + 3):
                if n_before + n_new == 0:
                    continue   # a final call with nothing pushed is refused before the scheduler
                k = gpt_windows_run(n_before, S, H_g)
                n, total = n_before, 0
                for take, held, k_first, n_win, fw, fids in gpt_stream_rounds(n_before, n_new, True, S, H_g):
                    assert k_first == k and held == n - k * H_g and 0 <= held <= S and held + take <= 2 * S
                    n, k, total = n + take, k + n_win, total + take
                    assert k == gpt_windows_run(n, S, H_g) and (k == k_first or (k - 1 - k_first) * H_g + S < held + take)
                    assert not fw or (fids == n - k * H_g and 1 <= fids <= S)
                assert total == n_new and (n == 0 or fw)


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------------
def test_both_draws_are_prefixes_of_the_offline_draws_however_they_are_chunked():
    for seed in (0, 2024):
        whole = semantic_decoder.seeded_uniforms(seed, 1, 3000)[0]
        for cap in (1, 10, 34, 1024, 2999):
            assert np.array_equal(semantic_decoder.seeded_uniforms(seed, 1, cap)[0], whole[:cap]), "prefix-stable in cap"
        d = _Draws(seed, 1)
        for lo, hi in ((0, 24), (24, 36), (36, 37), (37, 1500), (1500, 3000)):
            assert np.array_equal(d.rows(lo, hi).reshape(-1), whole[lo:hi]), "and under chunked draws on one generator"
        for W in WINDOWS:
            fine = fine_decoder.seeded_uniforms(seed, 1, 9, W)[0]
            for n in (1, 2, 5):
                assert np.array_equal(fine_decoder.seeded_uniforms(seed, 1, n, W)[0], fine[:n]), "prefix-stable in n"
            d = _Draws(seed, 6 * W)
            for lo, hi in ((0, 1), (1, 2), (2, 6), (6, 9)):
                assert np.array_equal(d.rows(lo, hi).reshape(-1, 6, W), fine[lo:hi])


def test_explicit_draws_that_run_out_raise():
    d = _Draws(0, 1, np.zeros(10, dtype=np.float32))
    assert d.rows(0, 10).shape == (10, 1)
    with pytest.raises(ValueError, match="needs entry 10"):
        d.rows(4, 11)


# ---- the twins chained ---------------------------------------------------------------------------------------------------------------------------------
def test_the_twins_under_the_stream_schedule_equal_the_offline_twins():
    """One short source on K.CFG and fine model "a": the GPT twin and the fine twin, run when the stream's rule lets them, give the ids and codes of
    ``twin_chain`` and ``fine_ref.generate``: the rule itself, not the device, is equal."""
    w, fw = K.weights("uniform"), fine_cases.weights("a", "uniform")
    N = K.S + K.H + 1
    src = K.source(N, seed=3)
    u = K.draws([N], K.MAX_NEW)[0]
    want_stream, want_finish, _ = K.twin_chain(w, K.CFG, src, u)
    T = len(want_stream) // 2
    assert T >= 1
    fu = fine_decoder.seeded_uniforms(7, 1, len(fine_ref.fine_windows(T, 128)), 128)[0]
    codes = np.stack([want_stream[0:2 * T:2] - K.CFG.ACOUSTIC_OFFSET, want_stream[1:2 * T:2] - K.CFG.ACOUSTIC_OFFSET - K.CFG.codebook_size])
    want_codes, _ = fine_ref.generate(fw, codes, 0.5, fu)
    for name, pushes in SC.splittings(N, K.S, K.H).items():
        if name == "ones":
            continue   # the same windows as "past_window", one id at a time
        stream, finish, got, events = SC.stream_twin(w, K.CFG, fw, src, pushes, u, fu)
        assert np.array_equal(stream, want_stream) and finish == want_finish, name
        assert np.array_equal(got, want_codes), name
        sched = stream_schedule(pushes, K.S, K.H, K.r, K.BLOCK, 128, final_budget_result=events[-1]["made"], max_new_tokens=K.MAX_NEW)
        assert [e["new_ids"] for e in sched] == [e["made"] for e in events] and [e["frames"] for e in sched] == [e["frames"] for e in events]


# ---- the library's host side ---------------------------------------------------------------------------------------------------------------------------
def run_tool(args=""):
    cmd = ["make", "-s", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "semantic_stream_asan"] + (["STREAM_ARGS=" + args] if args else [])
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "AddressSanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
    return out.stdout


def test_refusals_under_the_sanitizers():
    assert "semantic stream argument checks: ok" in run_tool()


def rounds_of(stdout):
    pushes = []
    for line in stdout.split("\n"):
        if line.startswith("push "):
            pushes.append([])
        elif line.startswith("round "):
            pushes[-1].append(tuple(int(x) for x in line.split()[1:]))
    return pushes


def test_the_librarys_schedulers_equal_the_twins_round_for_round():
    run_tool()   # builds it once
    for S, H_g in [(8, 4), (16, 8), (250, 124)]:
        calls = [(b, n, f) for b in (0, 1, S, S + 1, S + H_g, 3 * S + 5) for n in (0, 1, H_g, 2 * S, 2 * S + 1, 9 * S + 2) for f in (0, 1) if b + n > 0 or not f]
        got = rounds_of(run_tool(f"gpt {S} {H_g} " + " ".join(f"{b}:{n}:{f}" for b, n, f in calls)))
        assert got == [gpt_stream_rounds(b, n, bool(f), S, H_g) for b, n, f in calls]
    for W in (128, 256, 1024):
        H = W // 2
        calls = [(b, n, f) for b in (0, 1, W - 1, W, W + H, 2 * W + 3) for n in (0, 1, H, W, 2 * W, 2 * W + 1, 5 * W + 7) for f in (0, 1) if b + n > 0 or not f]
        got = rounds_of(run_tool(f"fine {W} " + " ".join(f"{b}:{n}:{f}" for b, n, f in calls)))
        assert got == [fine_stream_rounds(b, n, bool(f), W) for b, n, f in calls]
