"""Writes tests/golden/fine_a.npz: what an independent implementation of the fine stage, ``transformers``' ``BarkFineModel`` and its ``generate``, computes
for two small seeded models (``weights.synth_fine_weights``). Results only, no weights. tests/test_oracle_fine_cpu.py pins tests/fine_ref.py to it.

    python tests/golden/make_golden_fine.py        (CPU, a few seconds)

Per model ``m`` in (a: W = 128, 2 layers, E = 768, no linear biases; b: W = 256, 1 layer, E = 1024, biases):
  m_buf [W, 8], m_pos [24], m_logits_c{2,5,7} [24, 1024]   logits of three forwards of one seeded buffer at 24 positions
  m_T [8]; per T: m_coarse_T [2, T], m_codes_T [8, T]      ``generate`` on the argmax path (temperature None)
                  m_sched_T [n, 2]                          the (start, fill) of every window HF walked
                  m_ids_T [n, 6, W]                         the id every pass wrote (-1 below rel), overwritten ones included
                  m_margin_T [n, 6, W]                      the top-2 margin of the logits each id is the argmax of (inf below rel)
HF's loop exposes neither ``start`` nor ``rel``: the script reads them off the run itself. ``start`` is the storage offset of the buffer view that
``forward`` receives (a slice of the ``[1, L, 8]`` work tensor), ``rel`` is ``W`` minus the number of positions handed to ``torch.argmax``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from audiotoken_amd import weights as Wt   # noqa: E402

MODELS = {"a": dict(block=128, n_layer=2, hidden=768, bias=False), "b": dict(block=256, n_layer=1, hidden=1024, bias=True)}
FAMILY = "peaky"
HF_PARTS = ((".ln_1.", ".layernorm_1."), (".ln_2.", ".layernorm_2."), (".attn.c_attn.", ".attn.att_proj."), (".attn.c_proj.", ".attn.out_proj."),
            (".mlp.c_fc.", ".mlp.in_proj."), (".mlp.c_proj.", ".mlp.out_proj."))
HF_HEADS = (("transformer.wtes.", "input_embeds_layers."), ("transformer.wpe.", "position_embeds_layer."), ("transformer.ln_f.", "layernorm_final."),
            ("transformer.h.", "layers."))


def lengths(W):
    H = W // 2
    return [1, H, W - 1, W, W + 1, W + H, W + H + 1, 2 * W + 3]


def coarse_of(T, W):
    return np.random.default_rng(1000 * W + T).integers(0, 1024, size=(2, T))


def hf_model(w, block, n_layer, hidden, bias):
    from transformers.models.bark.configuration_bark import BarkFineConfig
    from transformers.models.bark.modeling_bark import BarkFineModel
    cfg = BarkFineConfig(block_size=block, input_vocab_size=1056, output_vocab_size=1056, num_layers=n_layer, num_heads=hidden // 64, hidden_size=hidden,
                         dropout=0.0, bias=bias, n_codes_total=8, n_codes_given=1, tie_word_embeddings=False)
    model = BarkFineModel(cfg).eval()
    sd = {}
    for k, v in w.items():
        for ours, hf in HF_HEADS:
            if k.startswith(ours):
                k = hf + k[len(ours):]
                break
        for ours, hf in HF_PARTS:
            k = k.replace(ours, hf)
        sd[k] = torch.from_numpy(v)
    missing, unexpected = model.load_state_dict(sd, strict=False)
    assert not unexpected and all(m.endswith(".attn.bias") for m in missing), (missing, unexpected)
    return model


def hf_generate(model, coarse, W):
    """(codes [8, T], [(start, fill)], ids [n, 6, W], top-2 margins [n, 6, W]) of HF's generate on the argmax path."""
    from transformers.models.bark.generation_configuration_bark import (BarkCoarseGenerationConfig, BarkFineGenerationConfig,
                                                                         BarkSemanticGenerationConfig)
    sem = BarkSemanticGenerationConfig(semantic_vocab_size=0)          # generate subtracts it from the coarse ids before the remainder by 1024
    coa = BarkCoarseGenerationConfig(n_coarse_codebooks=2)
    fin = BarkFineGenerationConfig(temperature=None, max_fine_history_length=W // 2, max_fine_input_length=W, n_fine_codebooks=8)
    starts, rels, margins, ids = [], [], [], []
    forward, argmax = model.forward, torch.argmax

    def spy_forward(codebook_idx, input_ids, *a, **kw):
        if codebook_idx == 2:
            assert input_ids.shape[0] == 1 and input_ids.stride() == (input_ids.stride(0), 8, 1)
            starts.append(input_ids.storage_offset() // 8)
        return forward(codebook_idx, input_ids, *a, **kw)

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
                                 fine_generation_config=fin, codebook_size=1024, temperature=None)
    finally:
        model.forward, torch.argmax = forward, argmax
    assert len(rels) == 6 * len(starts) and all(len(set(rels[6 * k:6 * k + 6])) == 1 for k in range(len(starts)))
    sched = [(s, s + rels[6 * k]) for k, s in enumerate(starts)]
    n = len(starts)
    return out[0].numpy().astype(np.int16), np.array(sched, dtype=np.int32), np.stack(ids).reshape(n, 6, W), np.stack(margins).reshape(n, 6, W)


def main():
    torch.manual_seed(0)
    out = {}
    for name, m in MODELS.items():
        W = m["block"]
        w = Wt.synth_fine_weights(m["n_layer"], m["hidden"], W, seed=0, family=FAMILY, bias=m["bias"])
        model = hf_model(w, **m)
        rng = np.random.default_rng(17 + W)
        buf = rng.integers(0, 1024, size=(W, 8))
        buf[rng.random((W, 8)) < 0.1] = 1024        # cells that hold nothing yet, in every channel
        pos = np.sort(rng.choice(W, size=24, replace=False))
        pos[0], pos[-1] = 0, W - 1
        out[f"{name}_buf"], out[f"{name}_pos"] = buf.astype(np.int16), pos.astype(np.int16)
        for c in (2, 5, 7):
            with torch.no_grad():
                logits = model(c, torch.from_numpy(buf)[None]).logits[0]
            out[f"{name}_logits_c{c}"] = logits[torch.from_numpy(pos)][:, :1024].numpy().astype(np.float32)
        out[f"{name}_T"] = np.array(lengths(W), dtype=np.int32)
        for T in lengths(W):
            coarse = coarse_of(T, W)
            codes, sched, ids, margin = hf_generate(model, coarse, W)
            assert codes.shape == (8, T) and np.array_equal(codes[:2], coarse)
            print(f"model {name} T {T}: {len(sched)} windows {sched.tolist()}, smallest margin {margin.min():.3e}, {int((margin < 1e-3).sum())} below 1e-3")
            out[f"{name}_coarse_{T}"], out[f"{name}_codes_{T}"] = coarse.astype(np.int16), codes
            out[f"{name}_sched_{T}"], out[f"{name}_ids_{T}"], out[f"{name}_margin_{T}"] = sched, ids, margin
    path = os.path.join(ROOT, "tests", "golden", "fine_a.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
