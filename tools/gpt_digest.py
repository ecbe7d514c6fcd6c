#!/usr/bin/env python3
"""One sha256 per output of a fixed, seeded table of GPT generation calls, through the public Python API only: the bit-identity
check of a change to the decoder's bookkeeping or host code that must not change results. Run it on two library builds on the same machine and diff:

    python tools/gpt_digest.py > a.txt        # AUDIOTOKEN_HIP_LIB selects the library, as everywhere

Every model is the 2-layer synthetic one at V = 2048 (tests/long_form_cases.py), in both weight families, `uniform` and `peaky`. The table:
``generate`` across the route switch at block 128 (one row of 1, 63, 64, 65 tokens; rows of 16 16 16 16 and 16 16 16 17, a pass of 64 and of 65 tokens;
17 rows, a second pass of the linear kernel) and its bookkeeping at block 64 (a row born finished beside a running one, a stop token that hits,
``max_new`` 16 and 17 around the host's poll, allow sets, a prompt id outside the vocabulary); ``to_acoustic_long`` at block 64, S = 8, H = 4 on
``LENGTHS`` singly and on the ``MIXED_ROWS`` batch, lockstep and with ``slots`` 1 and 4; block 128, S = 16, H = 8 through 8 slots with mixed ticks on
both routes; ``tick_tokens`` at its minimum; the prompted long form (tests/voice_cases.py: every ``PROMPTS`` length on the ``TOTALS``, one
shared prompt and one per row with rows that have none), lockstep and with ``slots``; ``top_p`` / ``min_p`` on ``generate`` and on the long
form; ``score_acoustic``, short and ``long_form=True``, with its logits. Per call: ids, ``last_raw_ids``, lengths, finish reasons, logits,
the status word, for the queue ``ticks`` and ``placement``, for a score log-probs, ranks, ``last_raw_scores`` and logits. Last, the value of every size
query of the handle for a fixed table of shapes, refused ones (0) among them. A few seconds in all."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, acoustic_windows, queue_ticks, seeded_uniforms, stream_extent  # noqa: E402
from tests import gpt_queue_cases as Q  # noqa: E402
from tests import long_form_cases as K  # noqa: E402
from tests import voice_cases as VC  # noqa: E402


def sha(x) -> str:
    if isinstance(x, (list, tuple)) and x and isinstance(x[0], torch.Tensor):
        x = b"".join(t.detach().contiguous().cpu().numpy().tobytes() + b"|" for t in x)
    elif isinstance(x, torch.Tensor):
        x = x.detach().contiguous().cpu().numpy().tobytes()
    elif not isinstance(x, bytes):
        x = repr(x).encode()
    return hashlib.sha256(x).hexdigest()[:32]


def line(name: str, dec, **outputs) -> None:
    print(f"{name:58s} status={dec.last_status()} " + " ".join(f"{k}={sha(v)}" for k, v in outputs.items()), flush=True)


def prompt(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(7919 * seed + n).integers(0, K.V, size=n).astype(np.int32)


def generate(name, dec, prompts, max_new, **kw) -> None:
    u = seeded_uniforms(len(prompts) + max_new, len(prompts), max_new)
    try:
        ids, finish, logits = dec.generate(prompts, max_new_tokens=max_new, temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True, **kw)
    except ValueError as e:
        line(name, dec, raised=str(e))
        return None
    line(name, dec, ids=ids, last_raw_ids=dec.last_raw_ids, out_len=[len(i) for i in ids], finish=finish, logits=logits)
    return ids


def long_form(name, dec, case, srcs, u, **kw) -> None:
    try:
        out = dec.to_acoustic_long([torch.from_numpy(s) for s in srcs], window=case["S"], hop=case["H"], max_new_tokens=case["max_new"],
                                   temperature=K.TEMPERATURE, top_k=K.TOP_K, uniforms=u, return_logits=True, **kw)
    except ValueError as e:
        line(name, dec, raised=str(e))
        return
    line(name, dec, ids=out.ids, last_raw_ids=dec.last_raw_ids, out_len=[len(i) for i in out.ids], finish=out.finish, logits=out.logits, windows=out.windows,
         ticks=out.ticks, placement=out.placement)


def score(name, dec, srcs, codes, **kw) -> None:
    try:
        sc = dec.score_acoustic(srcs, codes, temperature=K.TEMPERATURE, return_logits=True, **kw)
    except ValueError as e:
        line(name, dec, raised=str(e))
        return
    line(name, dec, logprob=sc.logprob, rank=sc.rank, nll=sc.nll, windows=sc.windows, logits=sc.logits, last_raw_scores=list(dec.last_raw_scores))


def state_sizes(fam: str, dec) -> None:
    """Every size query of the handle on a fixed table of shapes: the smallest, the largest, some between, and some that are refused (0)."""
    table = {
        "state_bytes": [(1, 1), (1, 128), (17, 64), (64, 128), (0, 1), (1, 129)],
        "long_state_bytes": [(1, 1), (1, 128), (17, 64), (64, 128), (65, 1), (1, 0)],
        "queue_state_bytes": [(1, 64, 65), (4, 64, 200), (8, 128, 1032), (64, 128, 65600), (4, 64, 67), (4, 64, 65601)],
        "score_state_bytes": [(1, 2, 2, 16), (8, 64, 512, 1024), (64, 128, 65600, 4096), (8, 64, 63, 1024), (8, 64, 512, 24)],
        "stream_state_bytes": [(2, 2, 1), (8, 4, 3), (16, 8, 3), (30, 30, 3), (32, 16, 3), (8, 10, 3)],
    }
    for fn, shapes in table.items():
        print(f"{fam} at_gpt_{fn} " + " ".join(f"{a}={int(dec._fn(fn)(dec.handle, *a))}" for a in shapes), flush=True)


def max_len_of(case) -> int:
    plans = [acoustic_windows(N, case["S"], case["H"], K.r, case["block"]) for N in case["lens"]]
    return stream_extent(plans, case["S"], K.r, case["max_new"], case["block"])[2]


def family(fam: str) -> None:
    # ---- generate: the route switch
    dec = SemanticToAcoustic(K.CFG, device="cuda:0", weights=K.weights(fam, block=128))
    for n in (1, 63, 64, 65):
        generate(f"{fam} generate one row of {n}", dec, [prompt(n, 1)], 6)
    generate(f"{fam} generate rows 16 16 16 16", dec, [prompt(16, 10 + b) for b in range(4)], 6)
    generate(f"{fam} generate rows 16 16 16 17", dec, [prompt(16 + b // 3, 20 + b) for b in range(4)], 6)
    generate(f"{fam} generate 17 rows", dec, [prompt(3 + b, 30 + b) for b in range(17)], 6)
    # ---- generate: the bookkeeping
    dec = SemanticToAcoustic(K.CFG, device="cuda:0", weights=K.weights(fam))
    generate(f"{fam} generate a row born finished", dec, [prompt(K.BLOCK, 40), prompt(5, 41)], 8)
    ids = generate(f"{fam} generate no stop token", dec, [prompt(9, 50), prompt(4, 51)], 8)
    generate(f"{fam} generate a stop token that hits", dec, [prompt(9, 50), prompt(4, 51)], 8, stop_token=int(ids[0][2]))
    for max_new in (16, 17):
        generate(f"{fam} generate max_new {max_new}", dec, [prompt(7, 60), prompt(47, 61), prompt(48, 62)], max_new)
    generate(f"{fam} generate allow sets", dec, [prompt(6, 70), prompt(11, 71)], 9, allow=K.allow_of(K.CFG, True), stop_token=K.CFG.STOP_TOKEN)
    bad = prompt(6, 80)
    bad[3] = K.V + 5
    generate(f"{fam} generate a prompt id out of range", dec, [bad, prompt(3, 81)], 4)
    # ---- the long form and the queue at block 64, S = 8, H = 4
    small = dict(S=K.S, H=K.H, block=K.BLOCK, max_new=K.MAX_NEW)
    for slots in (None, 1, 4):
        kw, tag = ({}, "lockstep") if slots is None else (dict(slots=slots), f"slots={slots}")
        for N in K.LENGTHS:
            long_form(f"{fam} long N={N} {tag}", dec, small, [K.source(N, seed=1)], K.draws([N], K.MAX_NEW), **kw)
        long_form(f"{fam} long mixed rows {tag}", dec, small, [K.source(N, seed=2 + i) for i, N in enumerate(K.MIXED_ROWS)], K.draws(K.MIXED_ROWS, K.MAX_NEW), **kw)
    case = Q.CASES["mixed"]
    srcs, u = Q.inputs("mixed")
    long_form(f"{fam} queue tick_tokens at its minimum", dec, case, srcs, u, slots=4, tick_tokens=4 + max_len_of(case))
    # ---- block 128, S = 16, H = 8, 8 slots: the smallest tick_tokens at which a mixed tick runs on each route
    case = Q.CASES["routes"]
    dec = SemanticToAcoustic(K.CFG, device="cuda:0", weights=K.weights(fam, block=128))
    srcs, u = Q.inputs("routes")
    mixed = lambda ticks, route: [t for t in ticks if t[0] > 0 and t[2] > 0 and t[3] == route]
    for c in (1, 2, 4, 8):
        tick_tokens = 8 + c * max_len_of(case)
        predicted, _ = queue_ticks(case["lens"], 16, 8, K.r, 128, case["max_new"], 8, tick_tokens)
        if mixed(predicted, 1) and mixed(predicted, 0):
            break
    long_form(f"{fam} queue both routes tick_tokens={tick_tokens}", dec, case, srcs, u, slots=8, tick_tokens=tick_tokens)
    state_sizes(fam, dec)
    # ---- truncation on generate (block 128), then everything else at block 64, S = 8, H = 4
    for trunc in (dict(top_p=0.9), dict(min_p=0.05), dict(top_p=0.7, min_p=0.01)):
        generate(f"{fam} generate {trunc}", dec, [prompt(7, 90), prompt(65, 91)], 9, **trunc)
    dec = SemanticToAcoustic(K.CFG, device="cuda:0", weights=K.weights(fam))
    mixed_srcs = [K.source(N, seed=2 + i) for i, N in enumerate(K.MIXED_ROWS)]
    for trunc in (dict(top_p=0.9), dict(min_p=0.05), dict(top_p=0.7, min_p=0.01)):
        for kw, tag in (({}, "lockstep"), (dict(slots=2), "slots=2")):
            long_form(f"{fam} long mixed rows {trunc} {tag}", dec, small, mixed_srcs, K.draws(K.MIXED_ROWS, K.MAX_NEW), **trunc, **kw)
    # ---- the prompted long form: one prompt for every row, then a prompt, another and none by turns
    for kw, tag in (({}, "lockstep"), (dict(slots=1), "slots=1"), (dict(slots=3), "slots=3")):
        for P in VC.PROMPTS:
            rows = [(P, total - P) for total in VC.TOTALS if total - P >= 1]
            srcs = [K.source(N, seed=40 + i) for i, (_, N) in enumerate(rows)]
            long_form(f"{fam} prompted P={P} {tag}", dec, small, srcs, VC.draws(rows, K.MAX_NEW), voice=VC.prompt(P, seed=3), **kw)
        voices = [VC.prompt(VC.PROMPTS[i % 3], seed=i) if i % 3 < 2 else None for i in range(len(VC.TOTALS))]
        rows = [(0 if v is None else len(v), total - (0 if v is None else len(v))) for v, total in zip(voices, VC.TOTALS)]
        srcs = [K.source(N, seed=50 + i) for i, (_, N) in enumerate(rows)]
        long_form(f"{fam} prompted by turns {tag}", dec, small, srcs, VC.draws(rows, K.MAX_NEW), voice=voices, **kw)
    # ---- scoring: given codes, short (one row a source) and long (one row a window), and through more than one pass and head chunk
    rng = np.random.default_rng(17)
    short = [K.source(N, seed=60) for N in (1, 5, K.S)]
    codes = [torch.from_numpy(rng.integers(0, K.CFG.codebook_size, size=(2, T))) for T in (1, 20, 26)]
    score(f"{fam} score short", dec, short, codes)
    score(f"{fam} score short constrained no stop", dec, short, codes, constrain=True, include_stop=False)
    score(f"{fam} score short two rows a pass", dec, short, codes, rows=2, head_rows=16)
    codes = [torch.from_numpy(rng.integers(0, K.CFG.codebook_size, size=(2, K.capacity(N, 6) // 2))) for N in K.MIXED_ROWS]
    score(f"{fam} score long", dec, mixed_srcs, codes, long_form=True, window=K.S, hop=K.H)
    score(f"{fam} score long small passes", dec, mixed_srcs, codes, long_form=True, window=K.S, hop=K.H, rows=3, pass_tokens=K.BLOCK, head_rows=32)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device"
    for fam in K.FAMILIES:
        family(fam)
