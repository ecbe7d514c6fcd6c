"""Writes tests/golden/fine_hist_a.npz: what ``transformers``' ``BarkFineModel.generate`` computes WITH ``history_prompt["fine_prompt"]`` for the two small
seeded models of make_golden_fine.py (whose model builder and spies this script reuses). Results only, no weights. tests/test_fine_history_cpu.py pins
tests/fine_hist_ref.py to it.

    python tests/golden/make_golden_fine_history.py        (CPU, under a minute)

The argmax path only (``temperature=None``): HF's sampling branch slices the logits twice where ``rel > 0`` and is no authority there.
Per model ``m`` in (a, b), with H = W / 2 and h = min(H, Th):
  m_Th [4] = 1, H - 1, H, H + 5;  m_hist_{Th} [8, Th]             the history prompts
  per Th, m_T_{Th} [5] = 1, W - h - 1, W - h, W - h + 1, W + H + 1; per (Th, T), with key = "{Th}_{T}":
    m_coarse_key [2, T], m_codes_key [8, T]    the row and HF's result (the history is not part of it)
    m_sched_key [n, 2]                         the (start, fill) of every window HF walked
    m_ids_key [n, 6, W]                        the id every pass wrote (-1 below rel), overwritten ones included
    m_margin_key [n, 6, W] float16             the top-2 margin of the logits each id is the argmax of (inf below rel), rounded UP to float16, so that a
                                               margin recorded below 1e-3 was below it
    m_pos_key [3], m_logits_key [3, 1024]      window 0, code book 2: the logits at buffer positions rel, (rel + W) / 2 and W - 1"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from audiotoken_amd import weights as Wt   # noqa: E402
from make_golden_fine import FAMILY, MODELS, hf_model   # noqa: E402


def history_lengths(W):
    H = W // 2
    return [1, H - 1, H, H + 5]


def row_lengths(W, h):
    H = W // 2
    return [1, W - h - 1, W - h, W - h + 1, W + H + 1]


def coarse_of(T, Th, W):
    return np.random.default_rng(1000 * W + 7 * Th + T).integers(0, 1024, size=(2, T))


def history_of(Th, W):
    return np.random.default_rng(500 * W + Th).integers(0, 1024, size=(8, Th))


def round_up_f16(x):
    y = x.astype(np.float16)
    low = y.astype(np.float32) < x
    y[low] = np.nextafter(y[low], np.float16(np.inf))
    return y


def hf_generate(model, coarse, history, W):
    """(codes [8, T], [(start, fill)], ids [n, 6, W], margins [n, 6, W], positions [3], logits [3, 1024]) of HF's generate on the argmax path."""
    from transformers.models.bark.generation_configuration_bark import (BarkCoarseGenerationConfig, BarkFineGenerationConfig,
                                                                         BarkSemanticGenerationConfig)
    sem = BarkSemanticGenerationConfig(semantic_vocab_size=0)
    coa = BarkCoarseGenerationConfig(n_coarse_codebooks=2)
    fin = BarkFineGenerationConfig(temperature=None, max_fine_history_length=W // 2, max_fine_input_length=W, n_fine_codebooks=8)
    starts, rels, margins, ids, first = [], [], [], [], []
    forward, argmax = model.forward, torch.argmax

    def spy_forward(codebook_idx, input_ids, *a, **kw):
        if codebook_idx == 2:
            assert input_ids.shape[0] == 1 and input_ids.stride() == (input_ids.stride(0), 8, 1)
            starts.append(input_ids.storage_offset() // 8)
        out = forward(codebook_idx, input_ids, *a, **kw)
        if codebook_idx == 2 and len(starts) == 1:
            first.append(out.logits[0, :, :1024].clone())
        return out

    def spy_argmax(x, *a, **kw):
        top = torch.topk(x.double(), 2, dim=-1).values
        got = argmax(x, *a, **kw)
        rel = W - x.shape[1]
        margins.append(np.concatenate([np.full(rel, np.inf), (top[0, :, 0] - top[0, :, 1]).numpy()]).astype(np.float32))
        ids.append(np.concatenate([np.full(rel, -1), got[0].numpy()]).astype(np.int16))
        rels.append(rel)
        return got

    model.forward, torch.argmax = spy_forward, spy_argmax
    try:
        with torch.no_grad():
            out = model.generate(torch.from_numpy(coarse.T.reshape(1, -1).copy()), semantic_generation_config=sem, coarse_generation_config=coa,
                                 fine_generation_config=fin, codebook_size=1024, temperature=None,
                                 history_prompt={"fine_prompt": torch.from_numpy(history)})
    finally:
        model.forward, torch.argmax = forward, argmax
    assert len(rels) == 6 * len(starts) and all(len(set(rels[6 * k:6 * k + 6])) == 1 for k in range(len(starts)))
    sched = [(s, s + rels[6 * k]) for k, s in enumerate(starts)]
    n = len(starts)
    pos = np.array([rels[0], (rels[0] + W) // 2, W - 1])
    return (out[0].numpy().astype(np.int16), np.array(sched, dtype=np.int32), np.stack(ids).reshape(n, 6, W), np.stack(margins).reshape(n, 6, W),
            pos.astype(np.int16), first[0][torch.from_numpy(pos)].numpy().astype(np.float32))


def main():
    torch.manual_seed(0)
    out = {}
    for name, m in MODELS.items():
        W = m["block"]
        H = W // 2
        w = Wt.synth_fine_weights(m["n_layer"], m["hidden"], W, seed=0, family=FAMILY, bias=m["bias"])
        model = hf_model(w, **m)
        out[f"{name}_Th"] = np.array(history_lengths(W), dtype=np.int32)
        for Th in history_lengths(W):
            h = min(H, Th)
            history = history_of(Th, W)
            out[f"{name}_hist_{Th}"] = history.astype(np.int16)
            out[f"{name}_T_{Th}"] = np.array(row_lengths(W, h), dtype=np.int32)
            for T in row_lengths(W, h):
                coarse = coarse_of(T, Th, W)
                codes, sched, ids, margin, pos, logits = hf_generate(model, coarse, history, W)
                assert codes.shape == (8, T) and np.array_equal(codes[:2], coarse)
                print(f"model {name} Th {Th} T {T}: {len(sched)} windows {sched.tolist()}, smallest margin {margin.min():.3e}, "
                      f"{int((margin < 1e-3).sum())} below 1e-3")
                key = f"{Th}_{T}"
                out[f"{name}_coarse_{key}"], out[f"{name}_codes_{key}"] = coarse.astype(np.int16), codes
                out[f"{name}_sched_{key}"], out[f"{name}_ids_{key}"], out[f"{name}_margin_{key}"] = sched, ids, round_up_f16(margin)
                out[f"{name}_pos_{key}"], out[f"{name}_logits_{key}"] = pos, logits
    path = os.path.join(ROOT, "tests", "golden", "fine_hist_a.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
