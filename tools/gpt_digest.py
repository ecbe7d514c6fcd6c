#!/usr/bin/env python3
"""One sha256 per output of a fixed, seeded table of GPT generation calls, through the public Python API only: the bit-identity
check of a change to the decoder's bookkeeping or host code that must not change results. Run it on two library builds on the same machine and diff:

    python tools/gpt_digest.py > a.txt        # AUDIOTOKEN_HIP_LIB selects the library, as everywhere

Every model is the 2-layer synthetic one at V = 2048 (tests/long_form_cases.py), in both weight families, `uniform` and `peaky`. The table:
``generate`` across the route switch at block 128 (one row of 1, 63, 64, 65 tokens; rows of 16 16 16 16 and 16 16 16 17, a pass of 64 and of 65 tokens;
17 rows, a second pass of the linear kernel) and its bookkeeping at block 64 (a row born finished beside a running one, a stop token that hits,
``max_new`` 16 and 17 around the host's poll, allow sets, a prompt id outside the vocabulary); ``to_acoustic_long`` at block 64, S = 8, H = 4 on
``LENGTHS`` singly and on the ``MIXED_ROWS`` batch, lockstep and with ``slots`` 1 and 4; block 128, S = 16, H = 8 through 8 slots with mixed ticks on
both routes; ``tick_tokens`` at its minimum. Per call: ids, ``last_raw_ids``, lengths, finish reasons, logits, the status word, and for the queue
``ticks`` and ``placement``. A few seconds in all."""
import hashlib
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from audiotoken_amd.semantic_decoder import SemanticToAcoustic, acoustic_windows, queue_ticks, seeded_uniforms, stream_extent  # noqa: E402
from tests import gpt_queue_cases as Q  # noqa: E402
from tests import long_form_cases as K  # noqa: E402


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
    out = dec.to_acoustic_long([torch.from_numpy(s) for s in srcs], window=case["S"], hop=case["H"], max_new_tokens=case["max_new"], temperature=K.TEMPERATURE,
                               top_k=K.TOP_K, uniforms=u, return_logits=True, **kw)
    line(name, dec, ids=out.ids, last_raw_ids=dec.last_raw_ids, out_len=[len(i) for i in out.ids], finish=out.finish, logits=out.logits, windows=out.windows,
         ticks=out.ticks, placement=out.placement)


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


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs a HIP device"
    for fam in K.FAMILIES:
        family(fam)
