"""What the CPU and the GPU tests of the generation queue share: the sources, seeds and geometry of every GPU case, so that
tests/test_gpt_queue_cpu.py can show on the twin alone that exactly these inputs do not lean on the sampling waiver. Everything else (the token space,
the twin, the window prompts) is tests/long_form_cases.py's."""
import numpy as np

from tests import long_form_cases as K

S, H, r = K.S, K.H, K.r

# name -> lengths, the seed of the sources (K.source(N, seed + i) for source i), the seed of the draws, the geometry, the final window's budget, the families
CASES = {
    "single":    dict(lens=list(K.LENGTHS), src_seed=20, u_seed=3001, S=S, H=H, block=K.BLOCK, max_new=K.MAX_NEW, families=K.FAMILIES),
    "reuse":     dict(lens=[2 * S + 3, 1], src_seed=30, u_seed=3002, S=S, H=H, block=K.BLOCK, max_new=K.MAX_NEW, families=K.FAMILIES),
    "mixed":     dict(lens=[1, S, S + 1, 2 * S + 3] * 3, src_seed=40, u_seed=3003, S=S, H=H, block=K.BLOCK, max_new=K.MAX_NEW, families=K.FAMILIES),
    "routes":    dict(lens=[35, 35, 35, 35, 1, 16, 17, 35, 9, 25, 33, 20, 1, 17, 30, 35, 24, 5], src_seed=60, u_seed=3004, S=16, H=8, block=128,
                      max_new=K.MAX_NEW, families=("peaky",)),
    "many":      dict(lens=[1 + (7 * i) % (2 * S + 3) for i in range(130)], src_seed=100, u_seed=3005, S=S, H=H, block=K.BLOCK, max_new=K.MAX_NEW,
                      families=("uniform",)),
    "stop":      dict(lens=[S - 1, S + 1, 2 * S + 3, S + H, 1, S + H + 1, S, 2 * S + 3, S + 1], src_seed=300, u_seed=3006, S=S, H=H, block=K.BLOCK,
                      max_new=K.MAX_NEW, families=("stop",)),
}
# the product geometry: too slow for the twin's uncached chain on a CPU (as in tests/test_long_form_cpu.py), so the GPU file alone uses it
PRODUCT = dict(lens=[375, 251, 30], src_seed=400, u_seed=3007, S=250, H=124, block=1024, max_new=16)


def stop_heavy_weights():
    """tests/test_long_form_gpu.py's STOP-heavy model: the STOP row of ``wte`` scaled by 30."""
    base = K.weights("peaky")
    wte = base["transformer.wte.weight"].copy()
    wte[K.CFG.STOP_TOKEN] *= 30.0
    return {**base, "transformer.wte.weight": wte}


def weights(family, block=K.BLOCK):
    return stop_heavy_weights() if family == "stop" else K.weights(family, block)


def inputs(case, cfg=K.CFG):
    """(sources, draws [n_src, L]) of a case."""
    c = CASES[case] if isinstance(case, str) else case
    srcs = [K.source(N, seed=c["src_seed"] + i, cfg=cfg) for i, N in enumerate(c["lens"])]
    u = K.draws(c["lens"], c["max_new"], seed=c["u_seed"], S=c["S"], H=c["H"], block=c["block"])
    return srcs, u


def final_steps(out):
    """Per source the sampler launches its final window took on the device: its new ids, plus one for a sampled STOP."""
    return [win[-1][3] + (1 if fin == "stop" else 0) for win, fin in zip(out.windows, out.finish)]
