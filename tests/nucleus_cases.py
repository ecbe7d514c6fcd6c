"""What the CPU and the GPU tests of the sampler's truncation share: the op's grid of random rows, the crafted rows, and the inputs of the
generation tests. Everything here is data and the twin (tests/nucleus_ref.py); nothing touches a device."""
import numpy as np

from tests import long_form_cases as K
from tests import nucleus_ref as N

LIST = 1024                      # csrc/gpt_model.hip: NUCLEUS_LIST, top-k sets up to this size finish in LDS, larger ones by the radix descent
WIDTHS = [1, 64, 1001, 2048, 53376, 65536]
TEMPERATURES = [1.0, 0.8, 0.05]
TOP_PS = [1e-6, 0.3, 0.9, 1.0 - 2.0 ** -20]
MIN_PS = [None, 0.05]
ROWS = 8
UNIFORMS = np.array([0.03, 0.17, 0.31, 0.46, 0.58, 0.71, 0.86, 0.97], dtype=np.float32)
WAIVER = 0.02                    # of a test's rows


def top_ks(V):
    return sorted({1, min(100, V), V})


LIVE = [16, 100, 101, 300, 1000, 1100, 3000]
SEED = 3                         # chosen so that at most half the waiver cap lies inside NUCLEUS_WINDOW (tests/test_nucleus_cpu.py)


def grid_rows(V):
    """8 rows that serve every (T, top_p, min_p, top_k) of the width. Row 0 is N(0, 4^2) over the whole width (N(0, 1) at 64 ids and fewer). Rows 1 to 7 have ``LIVE[i - 1]`` live ids
    (at most V) on a lattice of step 0.3 in [0, 7.8], so that they tie, and the rest 60 to 70 below, distinct and without weight. A dense tail of small
    weights always puts some G(x) / S_K within NUCLEUS_WINDOW of top_p = 1 - 2^-20; the lattice rows step over it (tests/test_nucleus_cpu.py counts)."""
    rng = np.random.default_rng(7919 * V + SEED)
    z = (rng.standard_normal((ROWS, V)) * (4.0 if V > 64 else 1.0)).astype(np.float32)   # (at 64 ids a spread of 4 has a tail of such weights too)
    for i, n in enumerate(LIVE):
        z[i + 1] = (-60.0 - 10.0 * rng.random(V)).astype(np.float32)
        live = rng.permutation(V)[:min(n, V)]
        z[i + 1, live] = (0.3 * rng.integers(0, 27, size=live.size)).astype(np.float32)
    return z


def grid(V):
    return [(T, k, p, q) for T in TEMPERATURES for k in top_ks(V) for p in TOP_PS for q in MIN_PS]


def two_plateaus(V, n_high, gap, side):
    """``n_high`` ids at 0 and the rest at ``-gap`` (spread over the row), with ``top_p`` 1e-3 below (``side`` -1: the lower plateau's G / S_K sits above
    top_p and the plateau goes) or above (+1: it stays) the mass of the upper plateau."""
    z = np.full(V, -gap, dtype=np.float32)
    z[np.linspace(0, V - 1, n_high).astype(int)] = 0.0
    hi = float(n_high)
    lo = (V - n_high) * np.exp(np.float64(np.float32(-gap)))
    return z, float(np.float32(hi / (hi + lo) + side * 1e-3))


def crafted():
    """``(name, logits [V], temperature, top_k, top_p, min_p, allow, u, kept expected or None)``. None of these may be waived: the CPU test shows that
    every one lies outside NUCLEUS_WINDOW."""
    rng = np.random.default_rng(11)
    out = []
    for V in (1001, 1040):   # 1001 values fit the list, 1040 tied values overflow it although top_k = 100 does not; the draw at the middle of a step
        out.append((f"all equal, V {V}", np.full(V, 1.5, dtype=np.float32), 1.0, 100, 0.5, None, None, 400.5 / V, V))
    one = np.full(2048, -50.0, dtype=np.float32)
    one[777] = 50.0
    for k in (100, 2048):
        out.append((f"all mass on one id, top_k {k}", one, 1.0, k, 0.9, None, None, 0.4, 1))
    for V, k in ((512, 512), (2048, 2048), (2048, 100)):   # the list, the descent, and ties at the top-k threshold that overflow the list
        for side, kept in ((-1, 40), (+1, V)):
            z, p = two_plateaus(V, 40, 3.0, side)
            out.append((f"two plateaus, V {V} top_k {k}, lower one {'goes' if side < 0 else 'stays'}", z, 1.0, k, p, None, None, 0.6125, kept))
    z = (rng.standard_normal(4096) * 3.0).astype(np.float32)
    z[::2] = -np.inf
    for k in (100, 4096):
        out.append((f"-inf entries, top_k {k}", z, 0.8, k, 0.9, None, None, 0.5, None))
    z = (rng.standard_normal(2048) * 3.0).astype(np.float32)
    out.append(("an allow range of width 1", z, 0.8, 100, 0.9, 0.05, (7, 8, 0, 0), 0.5, 1))
    out.append(("two allow ranges of width 1", z, 0.8, 100, 0.9999, None, (7, 8, 100, 101), 0.5, 2))
    out.append(("top_k binds", z, 1.0, 3, 0.9999, None, None, 0.5, 3))
    out.append(("top_p binds", z, 1.0, 100, 0.3, None, None, 0.5, None))
    out.append(("min_p binds", z, 1.0, 100, None, 0.05, None, 0.5, None))
    lmin = N.log_min_p(0.05)
    z = np.full(2048, -30.0, dtype=np.float32)
    z[5] = 0.0
    z[900] = lmin                                        # exactly at m + lmin: stays
    z[901] = np.nextafter(lmin, np.float32(-np.inf))     # one ulp below: goes
    out.append(("a value exactly at m + lmin", z, 1.0, 100, None, 0.05, None, 0.5, 2))
    out.append(("a value exactly at m + lmin, with the nucleus", z, 1.0, 100, 0.9999, 0.05, None, 0.5, 2))
    z = (rng.standard_normal(4096) * 2.0).astype(np.float32)
    for k in (LIST - 1, LIST, LIST + 1):                 # both sides of the switch between the list and the descent
        out.append((f"the path switch, top_k {k}", z, 1.0, k, 0.9, None, None, 0.5, None))
    t = z.copy()
    order = np.argsort(-t)
    t[order[990:1040]] = t[order[990]]                   # 50 equal values around rank 1000: K has 1040 values at top_k = 1000 and overflows the list
    out.append(("ties overflow the list", t, 1.0, 1000, 0.9999, None, None, 0.5, None))
    return out


# ---- generation ---------------------------------------------------------------------------------------------------------------------------------
TOP_P, MIN_P = 0.9, 0.02
GEN_STEPS = 40
GEN_PROMPTS = [3, 17, 64, 90]            # at_gpt_generate: four rows of their own prompt lengths
LONG_LENS = [9, 10, 11, 12]              # two windows each at (S, H) = (8, 4)
QUEUE_LENS = [9, 12, 5, 10, 8, 11]       # more sources than the 2 slots: the later ones are admitted mid-run
LONG_MAX_NEW = 16


def long_draws(lens):
    return K.draws(lens, LONG_MAX_NEW, seed=K.SEED + 24)


def sources(lens):
    return [K.source(n, seed=24) for n in lens]
