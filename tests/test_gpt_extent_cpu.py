"""CPU: the window geometry and the extent that the three GPT generators share (csrc/gpt.h: ``gpt_window``, ``gpt_extent``) against their
Python twins (semantic_decoder.py: ``acoustic_windows`` / ``window_steps`` / ``stream_extent``). The library's side is printed by the stand-alone program
tools/gpt_queue_args.hip in its ``extent`` mode, under the host sanitizers."""
import itertools
import os
import subprocess

import pytest

from audiotoken_amd.semantic_decoder import acoustic_windows, check_windows, stream_extent, window_steps

from tests.test_gpt_queue_cpu import run_tool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = 3
GEOMETRIES = [(8, 4), (8, 8), (16, 8), (250, 124)]
BLOCKS = [64, 128, 1024]
MAX_NEW = [1, 10, 1024]


def lengths(S, H):
    return [1, S - 1, S, S + 1, S + H, S + H + 1, 2 * S + 3, 1500]


def fits(S, H, block):
    try:
        check_windows(S, H, R, block)
    except ValueError:
        return False
    return True


CASES = [(S, H, block, max_new) for (S, H), block, max_new in itertools.product(GEOMETRIES, BLOCKS, MAX_NEW) if fits(S, H, block)]


@pytest.fixture(scope="module")
def exe():
    run_tool()   # builds it once
    return os.path.join(ROOT, "audiotoken_amd", "csrc", "build_asan", "gpt_queue_args")


def test_every_geometry_of_the_table_has_a_case():
    assert len(CASES) == 27 and {(S, H) for S, H, _, _ in CASES} == set(GEOMETRIES) and {b for _, _, b, _ in CASES} == set(BLOCKS)


@pytest.mark.parametrize("S,H,block,max_new", CASES)
def test_the_librarys_geometry_equals_the_twin(exe, S, H, block, max_new):
    lens = lengths(S, H)
    out = subprocess.run([exe, "extent"] + [str(x) for x in (S, H, R, block, max_new)] + [str(N) for N in lens], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stdout[-2000:] + out.stderr[-2000:]
    lines = out.stdout.split("\n")
    got_extent = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("extent ")]
    got_windows = [tuple(int(x) for x in l.split()[1:]) for l in lines if l.startswith("window ")]
    plans = [acoustic_windows(N, S, H, R, block) for N in lens]
    windows = []
    for i, plan in enumerate(plans):
        for k, ((start, n_ids, carry, new), (P, budget)) in enumerate(zip(plan, window_steps(plan, max_new, block))):
            assert start == k * H
            windows.append((i, k, n_ids, P, budget, 1 if new is None else 0, R * start + carry))
    _, cap, longest = stream_extent(plans, S, R, max_new, block)
    assert got_windows == windows
    assert got_extent == [(longest, cap)]   # need_len, need_stride


def test_the_tool_refuses_what_check_windows_refuses(exe):
    for (S, H), block in itertools.product(GEOMETRIES, BLOCKS):
        if not fits(S, H, block):
            bad = subprocess.run([exe, "extent", str(S), str(H), str(R), str(block), "10", "5"], capture_output=True, text=True, timeout=120)
            assert bad.returncode == 2 and "refused" in bad.stdout
