"""CPU: every case of tests/gemm_f32_cases.py takes the route it is in the table for, asked of the library itself (at_op_gemm_route: launch_gemm's
configuration choice and the kernel's own body predicate counted over the grid on the host — nothing is launched, no device is needed). A case that
silently falls onto another route fails HERE; tests/test_gemm_f32_routes_gpu.py then only has to run the table."""
import ctypes as C

import numpy as np
import pytest

from audiotoken_amd import _cabi
from tests import gemm_f32_cases as G

FAKE = {"X": 4096, "X2": 8192, "W": 12288, "bias": 16384, "C": 20480}   # addresses are never dereferenced by the route query


def route(c, N=None, **over):
    lib = _cabi.load()
    ptrs = dict(FAKE)
    if not c.bias:
        ptrs["bias"] = 0
    if c.residual:
        ptrs["R"] = 24576
    if c.row_mask:
        ptrs["mask"] = 28672
    d = G.fill_desc(_cabi.GemmDesc(), c, ptrs, N=N)
    for k, v in over.items():
        setattr(d, k, v)
    out = (C.c_int32 * 4)(-7, -7, -7, -7)
    rc = lib.at_op_gemm_route(C.byref(d), *G.dual_args(c, ptrs), out)
    return rc, list(out)


@pytest.mark.parametrize("c", G.CASES, ids=lambda c: c.name)
def test_case_reaches_the_pairs_it_claims(c):
    rc, (cfg, *counts) = route(c)
    assert rc == 0, _cabi.last_error()
    print(f"{c.name}: {G.CONFIG_NAMES[cfg]}  " + "  ".join(f"{G.BODY_NAMES[b]} {counts[b]}" for b in range(3)))
    assert c.routes, "a case must say what it is there for"
    for want_cfg, body in c.routes:
        assert (want_cfg, body) in G.REACHABLE
        assert cfg == want_cfg, f"{c.name}: configuration {G.CONFIG_NAMES[cfg]}, the table says {G.CONFIG_NAMES[want_cfg]}"
        assert counts[body] > 0, f"{c.name}: no workgroup takes the {G.BODY_NAMES[body]} body ({counts})"
    tiles = {G.C128x16: (128, 16), G.C128x32: (128, 32), G.C128x64: (128, 64), G.C128x64_K16: (128, 64), G.C64x64: (64, 64), G.C128x128_K16: (128, 128),
             G.C128x128: (128, 128)}[cfg]
    assert sum(counts) == -(-c.M // tiles[0]) * -(-c.N // tiles[1]) * c.batch, "the three counts cover the grid"


def test_table_covers_every_reachable_pair():
    seen = set()
    for c in G.CASES:
        rc, (cfg, *counts) = route(c)
        assert rc == 0
        seen |= {(cfg, b) for b in range(3) if counts[b] > 0}
    claimed = {p for c in G.CASES for p in c.routes}
    assert len(G.REACHABLE) == 18
    assert claimed == set(G.REACHABLE), f"pairs no case claims: {sorted(set(G.REACHABLE) - claimed)}"
    assert seen == set(G.REACHABLE), f"reached {sorted(seen)}: the model of reachable pairs and the library disagree"
    for name in sorted(G.REACHABLE):
        print(G.CONFIG_NAMES[name[0]], G.BODY_NAMES[name[1]])


def test_no_case_is_larger_than_it_needs_to_be():
    assert len({c.name for c in G.CASES}) == len(G.CASES)
    for c in G.CASES:
        assert c.out_bytes <= G.MAX_OUT_BYTES, c.name
        assert c.K <= G.MAX_K, c.name
    assert G.SOAK in G.BY_NAME and G.BY_NAME[G.SOAK].routes[0][0] == G.C128x128_K16
    assert G.BY_NAME[G.SOAK].out_bytes == max(c.out_bytes for c in G.CASES if c.routes[0][0] == G.C128x128_K16 and c.N == 3712)


def test_power_twins_take_another_body_or_configuration():
    """PRO_POWER has no im2col form: its bit-identity partner is the same launch with fewer columns, which must move the compared columns' last n-tile
    to another body (or the whole launch to another configuration)."""
    for c in G.CASES:
        if c.pro != G.PRO_POWER:
            continue
        assert 0 < c.twin_N < c.N
        _, (cfg, *counts) = route(c)
        rc, (tcfg, *tcounts) = route(c, N=c.twin_N)
        assert rc == 0
        assert tcfg != cfg or [n > 0 for n in tcounts] != [n > 0 for n in counts], c.name


def test_twin_chunks_stay_off_the_big_tiles():
    """The plain-Linear twin of a case runs at most 64 rows at a time: the 64x64 or a narrow configuration, never the case's own 128 x 128 one."""
    for c in G.CASES:
        if c.pro == G.PRO_POWER:
            continue
        twin = G.Case("twin", (), M=64, N=c.N, Cin=c.Cin if c.K2 else c.K, K2=c.K2, ld2=c.K2, pro=c.pro, epi=c.epi)
        rc, (cfg, *_) = route(twin)
        assert rc == 0 and cfg not in (G.C128x128, G.C128x128_K16), c.name


def test_route_query_refuses_what_the_launch_refuses():
    c = G.BY_NAME["dual_tap"]
    rc, out = route(c, K=c.Cin + 6)       # second source 6 wide
    assert rc == -1 and "multiple of 4" in _cabi.last_error()
    assert out == [-7, -7, -7, -7], "a refused query writes nothing"
    rc, out = route(G.BY_NAME["n32_k48"], M=0)
    assert rc == 0 and out == [-1, 0, 0, 0], "an empty launch has no configuration"


def test_builders_agree_with_each_other():
    """im2col (the twin's A) and operand64 (the float64 reference's A) are two statements of the same window rule."""
    for name in ("conv_min_clip", "conv_reflect_right", "conv_zero_right", "g48_grouped", "dual_general"):
        c = G.BY_NAME[name]
        t = G.build(c)
        a64, _ = G.operand64(c, t, c.batch - 1)
        assert np.array_equal(G.im2col(c, t, c.batch - 1, np.arange(c.M)).astype(np.float64), a64)
    c = G.BY_NAME["conv_min_clip"]            # rows m*2 + tap - 2 over a 3-row clip, reflected: (2,1,0,1), (0,1,2,1)
    r, ok = G.window_rows(c, [0, 1])
    assert r.tolist() == [[2, 1, 0, 1], [0, 1, 2, 1]] and ok.all()
    r, ok = G.window_rows(G.BY_NAME["conv_zero_right"], [0, 100])
    assert ok.tolist() == [[False, False, True, True], [True, True, True, False]]
