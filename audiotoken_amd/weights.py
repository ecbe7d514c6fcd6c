"""Weight dictionaries for the tokenizer models: synthetic generation and layout constants.

A model's weights are a flat ``dict[str, np.ndarray(float32)]`` whose keys follow the
checkpoint formats the reference loads, so a real checkpoint can be dropped in later
(SURVEY.md §8(f) N2):

* EnCodec 24 kHz — state-dict keys of ``encodec.EncodecModel.encodec_model_24khz()``
  (reference call site ``audiotoken/encoder.py:38``): ``encoder.model.{i}.conv.conv.{weight_g,
  weight_v,bias}``, ``encoder.model.{i}.block.{1,3}.conv.conv.*``, ``encoder.model.{i}.shortcut.conv.conv.*``,
  ``encoder.model.13.lstm.{weight_ih,weight_hh,bias_ih,bias_hh}_l{0,1}``,
  ``decoder.model.{i}.convtr.convtr.*``, ``quantizer.vq.layers.{k}._codebook.embed``.
* Wav2Vec2-BERT — HF ``Wav2Vec2BertModel`` state-dict keys (reference call site
  ``audiotoken/encoder.py:132``) plus ``vq._codebook.embed`` ``[1, 2048, 1024]``
  (``audiotoken/encoder.py:147-161``, ``audiotoken/utils.py:331-339``).

No pretrained weights exist offline, so benchmarks and parity tests use the synthetic
generators below (counter-based PRNG, bit-reproducible everywhere — see ``prng.py``).
"""
from __future__ import annotations

from typing import Dict, Optional, List, Tuple

import numpy as np

from . import prng

# ----------------------------------------------------------------------------------------------
# EnCodec 24 kHz architecture constants
# ----------------------------------------------------------------------------------------------
ENCODEC_RATIOS_ENC = (2, 4, 5, 8)      # encoder downsampling strides, in order
ENCODEC_RATIOS_DEC = (8, 5, 4, 2)      # decoder upsampling strides, in order
ENCODEC_FILTERS = 32
ENCODEC_DIM = 128
ENCODEC_CODEBOOK = 1024
ENCODEC_MAX_NQ = 32
ENCODEC_HOP = 320
ENCODEC_LSTM = 512


def encodec_conv_specs() -> List[Tuple[str, int, int, int, int]]:
    """(key prefix, c_in, c_out, kernel, stride) of every Conv1d of the SEANet *encoder*, in forward order."""
    specs = [("encoder.model.0.conv.conv", 1, ENCODEC_FILTERS, 7, 1)]
    c = ENCODEC_FILTERS
    idx = 1
    for r in ENCODEC_RATIOS_ENC:
        specs.append((f"encoder.model.{idx}.block.1.conv.conv", c, c // 2, 3, 1))
        specs.append((f"encoder.model.{idx}.block.3.conv.conv", c // 2, c, 1, 1))
        specs.append((f"encoder.model.{idx}.shortcut.conv.conv", c, c, 1, 1))
        specs.append((f"encoder.model.{idx + 2}.conv.conv", c, 2 * c, 2 * r, r))
        c *= 2
        idx += 3
    # idx == 13 -> LSTM, 14 ELU, 15 final conv
    specs.append(("encoder.model.15.conv.conv", c, ENCODEC_DIM, 7, 1))
    return specs


def encodec_decoder_specs() -> List[Tuple[str, str, int, int, int, int]]:
    """(kind, key prefix, c_in, c_out, kernel, stride) for the SEANet *decoder*; kind in {conv, convtr}."""
    c = ENCODEC_FILTERS * 16
    specs = [("conv", "decoder.model.0.conv.conv", ENCODEC_DIM, c, 7, 1)]
    idx = 3  # 1 = LSTM, 2 = ELU
    for r in ENCODEC_RATIOS_DEC:
        specs.append(("convtr", f"decoder.model.{idx}.convtr.convtr", c, c // 2, 2 * r, r))
        c //= 2
        specs.append(("conv", f"decoder.model.{idx + 1}.block.1.conv.conv", c, c // 2, 3, 1))
        specs.append(("conv", f"decoder.model.{idx + 1}.block.3.conv.conv", c // 2, c, 1, 1))
        specs.append(("conv", f"decoder.model.{idx + 1}.shortcut.conv.conv", c, c, 1, 1))
        idx += 3
    # idx == 15 -> ELU at 14, final conv at 15
    specs.append(("conv", "decoder.model.15.conv.conv", c, 1, 7, 1))
    return specs



# ----------------------------------------------------------------------------------------------
# weight families. "uniform" (rounds 1-4): every matrix U(-a, a) with variance 1 / fan_in, LayerNorm gains U(0.8, 1.2). "trained_like" (round 5) keeps
# every variance and emulates what published checkpoints look like where it matters for the two-piece fp16 arithmetic and for near-tie statistics:
# heavy-tailed matrices (tail index 4, largest entries 30-50 standard deviations out), log-normal LayerNorm / GroupNorm gains (sigma 0.5), a few
# "massive activation" channels (the same MASSIVE_CHANNELS indices in every layer: gain x 30-100 in the LayerNorm that writes the residual stream, and
# in every third layer also in the LayerNorm that feeds the first FFN GEMM), non-zero betas with a few large entries.
# ----------------------------------------------------------------------------------------------
FAMILIES = ("uniform", "trained_like")
N_MASSIVE = 3


def _family_check(family: str) -> bool:
    if family not in FAMILIES:
        raise ValueError(f"weight family {family!r}: one of {FAMILIES}")
    return family == "trained_like"


def massive_channels(model: str, dim: int, seed: int = 0) -> np.ndarray:
    """The N_MASSIVE channel indices of `model` that carry massive activations in the trained_like family."""
    u = prng.uniform01(f"{model}.massive_channels", 4 * N_MASSIVE, seed)
    idx = []
    for v in (u * dim).astype(np.int64):
        if int(v) not in idx:
            idx.append(int(v))
        if len(idx) == N_MASSIVE:
            break
    return np.asarray(idx, dtype=np.int64)


def _trained_ln(w, name: str, dim: int, seed: int, massive=None):
    g = prng.log_normal(name + ".weight", (dim,), 0.5, seed)
    b = prng.irwin_hall(name + ".bias", (dim,), 0.3, seed)
    big = (prng.uniform01(name + ".bias#big", dim, seed) < 4.0 / dim)          # ~4 betas of magnitude ~3
    b = np.where(big, np.sign(b) * np.float32(3.0) + b, b).astype(np.float32)
    if massive is not None:
        g = g.copy()
        g[massive] *= prng.uniform(name + ".weight#massive", (len(massive),), 30.0, 100.0, seed)
    w[name + ".weight"], w[name + ".bias"] = g.astype(np.float32), b


def _run_jobs(jobs):
    """Generate tensors on a thread pool (numpy releases the GIL inside its loops): jobs = [(key, fn)]; returns {key: array}."""
    import os
    from concurrent.futures import ThreadPoolExecutor
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:  # pragma: no cover
        n = os.cpu_count() or 1
    with ThreadPoolExecutor(max_workers=max(1, min(16, n))) as ex:
        return dict(zip([k for k, _ in jobs], ex.map(lambda kf: kf[1](), jobs)))

def _wn_pair(w: Dict[str, np.ndarray], prefix: str, shape, norm_dim0: int, seed: int, trained: bool = False):
    """weight_g / weight_v / bias for one weight-normalised conv. ``shape`` is the torch weight shape."""
    if trained:   # heavy-tailed direction, log-normal norm with the same median as the uniform family's mean
        w[f"{prefix}.weight_v"] = prng.heavy_tailed(f"{prefix}.weight_v", shape, 0.5773502691896258, seed)
        w[f"{prefix}.weight_g"] = prng.log_normal(f"{prefix}.weight_g", (norm_dim0, 1, 1), 0.35, seed, median=1.2)
        return
    w[f"{prefix}.weight_v"] = prng.uniform(f"{prefix}.weight_v", shape, -1.0, 1.0, seed)
    w[f"{prefix}.weight_g"] = prng.uniform(f"{prefix}.weight_g", (norm_dim0, 1, 1), 0.9, 1.5, seed)


def synth_encodec_weights(seed: int = 0, with_decoder: bool = True, n_codebooks: int = ENCODEC_MAX_NQ, family: str = "uniform") -> Dict[str, np.ndarray]:
    """Synthetic EnCodec-24kHz weights (encoder, RVQ codebooks, optionally decoder). family "trained_like": heavy-tailed weight_v / LSTM matrices /
    biases and log-normal weight_g (the variances of the uniform family are kept, so signal levels through the stack stay comparable)."""
    trained = _family_check(family)
    w: Dict[str, np.ndarray] = {}

    def bias(prefix, cout):
        w[f"{prefix}.bias"] = (prng.heavy_tailed(f"{prefix}.bias", (cout,), 0.0577, seed) if trained
                               else prng.uniform(f"{prefix}.bias", (cout,), -0.1, 0.1, seed))

    for prefix, cin, cout, k, _s in encodec_conv_specs():
        _wn_pair(w, prefix, (cout, cin, k), cout, seed, trained)
        bias(prefix, cout)
    a = 1.0 / np.sqrt(ENCODEC_LSTM)
    for which in ("encoder.model.13", "decoder.model.1"):
        if which.startswith("decoder") and not with_decoder:
            continue
        for layer in range(2):
            for nm, shape in (("weight_ih", (4 * ENCODEC_LSTM, ENCODEC_LSTM)), ("weight_hh", (4 * ENCODEC_LSTM, ENCODEC_LSTM)),
                              ("bias_ih", (4 * ENCODEC_LSTM,)), ("bias_hh", (4 * ENCODEC_LSTM,))):
                key = f"{which}.lstm.{nm}_l{layer}"
                w[key] = prng.heavy_tailed(key, shape, a / np.sqrt(3.0), seed) if trained else prng.uniform(key, shape, -a, a, seed)
    if with_decoder:
        for kind, prefix, cin, cout, k, _s in encodec_decoder_specs():
            if kind == "conv":
                _wn_pair(w, prefix, (cout, cin, k), cout, seed, trained)
            else:  # ConvTranspose1d weight is [in, out, k]; weight-norm dim 0 = input channel
                _wn_pair(w, prefix, (cin, cout, k), cin, seed, trained)
            bias(prefix, cout)
    for q in range(n_codebooks):
        key = f"quantizer.vq.layers.{q}._codebook.embed"
        scale = 1.2 * (0.75 ** q)
        w[key] = prng.irwin_hall(key, (ENCODEC_CODEBOOK, ENCODEC_DIM), scale, seed)
    return w


def fold_weight_norm(g: np.ndarray, v: np.ndarray) -> np.ndarray:
    """``W = g * v / ||v||`` with the norm over all dims but 0 (torch ``weight_norm(dim=0)``).

    Uses ``torch._weight_norm`` on the host — the very function torch's weight-norm parametrisation
    evaluates on every forward of the reference model — so the folded tensor handed to the device is
    bit-identical to the weight the reference convolves with on CPU.
    """
    import torch

    out = torch._weight_norm(torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)),
                             torch.from_numpy(np.ascontiguousarray(g, dtype=np.float32)), 0)
    return out.numpy()


# ----------------------------------------------------------------------------------------------
# synthetic waveforms (SURVEY.md §8(d) "synthetic inputs")
# ----------------------------------------------------------------------------------------------
def synth_waveform(n_clips: int, n_samples: int, sample_rate: int, seed: int = 1234, first_clip: int = 0) -> np.ndarray:
    """``float32 [n_clips, n_samples]`` in [-1, 1]: 0.3*sum of 4 sines (80..4000 Hz) + 0.05*noise, clipped.

    Clip ``i`` depends only on ``seed + first_clip + i`` so shards of a batch are reproducible per rank.
    """
    out = np.empty((n_clips, n_samples), dtype=np.float32)
    t = np.arange(n_samples, dtype=np.float64) / float(sample_rate)
    for i in range(n_clips):
        s = seed + first_clip + i
        f = 80.0 + 3920.0 * prng.uniform01("wave.freq", 4, s).astype(np.float64)
        ph = 2.0 * np.pi * prng.uniform01("wave.phase", 4, s).astype(np.float64)
        x = np.zeros(n_samples, dtype=np.float64)
        for j in range(4):
            x += np.sin(2.0 * np.pi * f[j] * t + ph[j])
        noise = prng.irwin_hall("wave.noise", (n_samples,), 1.0, s).astype(np.float64)
        out[i] = np.clip(0.3 * x + 0.05 * noise, -1.0, 1.0).astype(np.float32)
    return out


# ----------------------------------------------------------------------------------------------
# Wav2Vec2-BERT (semantic_m) — HF state-dict keys; architecture constants
# ----------------------------------------------------------------------------------------------
W2V_HIDDEN = 1024
W2V_FFN = 4096
W2V_HEADS = 16
W2V_HEAD_DIM = 64
W2V_FEAT = 160
W2V_DW_KERNEL = 31
W2V_REL_BUCKETS = 73          # left 64 + right 8 + 1
W2V_LAYERS_USED = 19          # hidden_states[19] = output of layer index 18 (reference encoder.py:172-175)
W2V_CODEBOOK = 2048


def synth_w2vbert_weights(n_layers: int = W2V_LAYERS_USED, seed: int = 0, with_vq: bool = True, family: str = "uniform") -> Dict[str, np.ndarray]:
    """Synthetic Wav2Vec2-BERT weights (first ``n_layers`` conformer layers) + the 2048 x 1024 VQ codebook. ``family``: see FAMILIES above."""
    trained = _family_check(family)
    w: Dict[str, np.ndarray] = {}
    jobs = []                      # trained_like: the big matrices are generated on a thread pool
    H, Fd = W2V_HIDDEN, W2V_FFN
    massive = massive_channels("w2vbert", H, seed) if trained else None

    def mat(name, shape, a):       # variance a^2 / 3 in both families
        if trained:
            jobs.append((name, lambda: prng.heavy_tailed(name, shape, a / np.sqrt(3.0), seed)))
        else:
            w[name] = prng.uniform(name, shape, -a, a, seed)

    def lin(name, out_f, in_f, bias=True, gain=1.0):
        mat(name + ".weight", (out_f, in_f), gain * np.sqrt(3.0 / in_f))
        if bias:
            w[name + ".bias"] = (prng.heavy_tailed(name + ".bias", (out_f,), 0.05, seed) if trained
                                 else prng.uniform(name + ".bias", (out_f,), -0.05, 0.05, seed))

    def ln(name, dim, massive_here=False):
        if trained:
            _trained_ln(w, name, dim, seed, massive if massive_here else None)
            return
        w[name + ".weight"] = prng.uniform(name + ".weight", (dim,), 0.8, 1.2, seed)
        w[name + ".bias"] = prng.uniform(name + ".bias", (dim,), -0.1, 0.1, seed)

    ln("feature_projection.layer_norm", W2V_FEAT)
    lin("feature_projection.projection", H, W2V_FEAT)
    for i in range(n_layers):
        p = f"encoder.layers.{i}"
        ln(p + ".ffn1_layer_norm", H, massive_here=(i % 3 == 1))
        lin(p + ".ffn1.intermediate_dense", Fd, H, gain=1.4)
        lin(p + ".ffn1.output_dense", H, Fd)
        ln(p + ".self_attn_layer_norm", H)
        for nm in ("linear_q", "linear_k", "linear_v", "linear_out"):
            lin(p + ".self_attn." + nm, H, H, gain=1.6 if nm in ("linear_q", "linear_k") else 1.0)
        mat(p + ".self_attn.distance_embedding.weight", (W2V_REL_BUCKETS, W2V_HEAD_DIM), 0.5)
        ln(p + ".conv_module.layer_norm", H)
        a = np.sqrt(3.0 / H)
        mat(p + ".conv_module.pointwise_conv1.weight", (2 * H, H, 1), 1.4 * a)
        mat(p + ".conv_module.depthwise_conv.weight", (H, 1, W2V_DW_KERNEL), np.sqrt(3.0 / W2V_DW_KERNEL))
        ln(p + ".conv_module.depthwise_layer_norm", H)
        mat(p + ".conv_module.pointwise_conv2.weight", (H, H, 1), a)
        ln(p + ".ffn2_layer_norm", H)
        lin(p + ".ffn2.intermediate_dense", Fd, H, gain=1.4)
        lin(p + ".ffn2.output_dense", H, Fd)
        ln(p + ".final_layer_norm", H, massive_here=True)      # this LayerNorm writes the residual stream the next layer reads
    if with_vq:
        # state-dict key of vector_quantize_pytorch.VectorQuantize (reference audiotoken/utils.py:331-339)
        w["vq._codebook.embed"] = prng.irwin_hall("vq._codebook.embed", (1, W2V_CODEBOOK, H), 1.0, seed)
    if jobs:
        made = _run_jobs(jobs)
        w = {**w, **made}
    return w


# ----------------------------------------------------------------------------------------------
# HuBERT-base (semantic_s, mHuBERT) — HF HubertModel state-dict keys (checkpoint naming: weight_g / weight_v for
# the positional conv); architecture constants
# ----------------------------------------------------------------------------------------------
HUB_CONV_KERNEL = (10, 3, 3, 3, 3, 2, 2)
HUB_CONV_STRIDE = (5, 2, 2, 2, 2, 2, 2)
HUB_CONV_DIM = 512
HUB_HIDDEN = 768
HUB_FFN = 3072
HUB_HEADS = 12
HUB_POS_K = 128
HUB_POS_GROUPS = 16
HUB_LAYERS_USED = 11          # hidden_states[11] (reference audiotoken/configs.py:53, encoder.py:95)
HUB_CENTROIDS = 1000


def hubert_num_frames(n_samples: int) -> int:
    """Chained valid-conv length formula floor((L - k)/s) + 1 (HF modeling_hubert.py:664-677)."""
    L = n_samples
    for k, s in zip(HUB_CONV_KERNEL, HUB_CONV_STRIDE):
        L = (L - k) // s + 1
    return L


def synth_hubert_weights(n_layers: int = HUB_LAYERS_USED, seed: int = 0, with_kmeans: bool = True, family: str = "uniform") -> Dict[str, np.ndarray]:
    trained = _family_check(family)
    w: Dict[str, np.ndarray] = {}
    jobs = []
    H, Fd, Cd = HUB_HIDDEN, HUB_FFN, HUB_CONV_DIM
    massive = massive_channels("hubert", H, seed) if trained else None

    def u(name, shape, a):
        if trained and len(shape) > 1:
            jobs.append((name, lambda: prng.heavy_tailed(name, shape, a / np.sqrt(3.0), seed)))
        elif trained:
            w[name] = prng.heavy_tailed(name, shape, a / np.sqrt(3.0), seed)
        else:
            w[name] = prng.uniform(name, shape, -a, a, seed)

    def lin(name, out_f, in_f, gain=1.0):
        u(name + ".weight", (out_f, in_f), gain * np.sqrt(3.0 / in_f))
        u(name + ".bias", (out_f,), 0.05)

    def ln(name, dim, massive_here=False):
        if trained:
            _trained_ln(w, name, dim, seed, massive if (massive_here and dim == H) else None)
            return
        w[name + ".weight"] = prng.uniform(name + ".weight", (dim,), 0.8, 1.2, seed)
        w[name + ".bias"] = prng.uniform(name + ".bias", (dim,), -0.1, 0.1, seed)

    cin = 1
    for i, k in enumerate(HUB_CONV_KERNEL):
        u(f"feature_extractor.conv_layers.{i}.conv.weight", (Cd, cin, k), 1.6 * np.sqrt(3.0 / (cin * k)))
        cin = Cd
    ln("feature_extractor.conv_layers.0.layer_norm", Cd)       # GroupNorm(512, 512) affine
    ln("feature_projection.layer_norm", Cd)
    lin("feature_projection.projection", H, Cd)
    u("encoder.pos_conv_embed.conv.weight_v", (H, H // HUB_POS_GROUPS, HUB_POS_K), 1.0)
    w["encoder.pos_conv_embed.conv.weight_g"] = prng.uniform("encoder.pos_conv_embed.conv.weight_g", (1, 1, HUB_POS_K), 1.5, 3.0, seed)
    u("encoder.pos_conv_embed.conv.bias", (H,), 0.05)
    ln("encoder.layer_norm", H)
    for i in range(n_layers):
        p = f"encoder.layers.{i}"
        for nm in ("q_proj", "k_proj", "v_proj", "out_proj"):
            lin(f"{p}.attention.{nm}", H, H, gain=1.6 if nm in ("q_proj", "k_proj") else 1.0)
        ln(p + ".layer_norm", H)
        lin(p + ".feed_forward.intermediate_dense", Fd, H, gain=1.4)
        lin(p + ".feed_forward.output_dense", H, Fd)
        ln(p + ".final_layer_norm", H, massive_here=True)      # post-LN: this LayerNorm writes the residual stream
    if with_kmeans:
        # sklearn KMeans.cluster_centers_ [1000, 768] (reference audiotoken/encoder.py:84-85)
        w["kmeans.cluster_centers_"] = prng.irwin_hall("kmeans.cluster_centers_", (HUB_CENTROIDS, H), 1.0, seed)
    if jobs:
        w = {**w, **_run_jobs(jobs)}
    if trained:
        # A post-LN stack hands its LayerNorm output — massive channels included — straight to the next layer's q / k projections. With RANDOM q / k weights
        # those three channels alone produce logits of several hundred: the softmax degenerates into an arg-max whose winner flips under the smallest
        # perturbation, and the network amplifies fp32 rounding noise 10 x per layer (measured, tools/family_probe.py + profiles/r05_family_probe_*.txt: the
        # float32 ORACLE then sits 0.5 from its own float64 evaluation in LayerNorm-normalised units at depth 11, and no two fp32 implementations agree on
        # the ids). Trained checkpoints are not chaotic: their q / k weights have learned the scale of those channels. Emulated here by dividing the q / k
        # columns of the massive channels by the gain the preceding LayerNorm gives them; v, out_proj and the FFN keep seeing the massive values (the range /
        # precision stress the family exists for). Conditioning after this: oracle32 vs oracle64 <= 5e-4 (uniform family: 5e-6).
        for i in range(1, n_layers):
            g = w[f"encoder.layers.{i - 1}.final_layer_norm.weight"][massive]
            for nm in ("q_proj", "k_proj"):
                key = f"encoder.layers.{i}.attention.{nm}.weight"
                w[key][:, massive] = (w[key][:, massive] / g[None, :]).astype(np.float32)
    return w


# ======================================================================================================
# HF checkpoint directories (save_pretrained layout) -> numpy state dict
# ======================================================================================================
GPT_FAMILIES = ("uniform", "peaky")


def synth_gpt_weights(n_layer: int = 12, vocab: int = 53376, block: int = 1024, seed: int = 0, family: str = "uniform") -> Dict[str, np.ndarray]:
    """Seeded synthetic weights of the semantic-to-acoustic GPT (csrc/gpt.hip) under the checkpoint's names. ``"uniform"`` is the nanoGPT initialisation:
    every matrix N(0, 0.02), the two ``c_proj`` at 0.02 / sqrt(2 n_layer); ``"peaky"`` is the same with ``wte`` at std 0.16, so that the logits spread
    over tens of units and top-k and the softmax see a real dynamic range. The LayerNorm gains are drawn from [0.8, 1.2] instead of the
    initialisation's ones, so that a kernel that dropped the gain would not pass."""
    if family not in GPT_FAMILIES:
        raise ValueError(f"weight family {family!r}: one of {GPT_FAMILIES}")
    E, F = 768, 3072
    proj_std = 0.02 / float(np.sqrt(2.0 * n_layer))
    jobs = [("transformer.wte.weight", (vocab, E), 0.16 if family == "peaky" else 0.02), ("transformer.wpe.weight", (block, E), 0.02)]
    for i in range(n_layer):
        p = f"transformer.h.{i}"
        jobs += [(f"{p}.attn.c_attn.weight", (3 * E, E), 0.02), (f"{p}.attn.c_proj.weight", (E, E), proj_std),
                 (f"{p}.mlp.c_fc.weight", (F, E), 0.02), (f"{p}.mlp.c_proj.weight", (E, F), proj_std)]
    w = _run_jobs([(name, (lambda name=name, shape=shape, std=std: prng.irwin_hall("gpt." + name, shape, std, seed))) for name, shape, std in jobs])
    for name in [f"transformer.h.{i}.ln_{j}.weight" for i in range(n_layer) for j in (1, 2)] + ["transformer.ln_f.weight"]:
        w[name] = prng.uniform("gpt." + name, (E,), 0.8, 1.2, seed)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def read_gpt_checkpoint(path) -> Dict[str, np.ndarray]:
    """The reference's stage-1 checkpoint as the tensors ``at_gpt_finalize`` takes: ``torch.load(path)["model"]``, an optional ``_orig_mod.`` prefix on
    every key, ``lm_head.weight`` tied to ``transformer.wte.weight``. Refused with ``ValueError``: biases, another ``n_embd``, an untied head."""
    import torch
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if not isinstance(ckpt, dict) or not isinstance(ckpt.get("model"), dict):
        raise ValueError(f"{path}: not a GPT checkpoint (a dict with a 'model' state dict is expected)")
    return gpt_tensors_from_state_dict(ckpt["model"], what=str(path))


def gpt_tensors_from_state_dict(sd, what: str = "state dict") -> Dict[str, np.ndarray]:
    pre = "_orig_mod."
    sd = {(k[len(pre):] if k.startswith(pre) else k): v for k, v in sd.items()}
    sd = {k: (v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32)) for k, v in sd.items()
          if not k.endswith(".attn.bias")}   # nanoGPT's causal-mask buffer is not a parameter
    biases = sorted(k for k in sd if k.endswith(".bias"))
    if biases:
        raise ValueError(f"{what}: the checkpoint has biases ({biases[0]}, ...); the HIP decoder implements the bias-free model only")
    wte = sd.get("transformer.wte.weight")
    if wte is None or wte.ndim != 2:
        raise ValueError(f"{what}: transformer.wte.weight is missing")
    if wte.shape[1] != 768:
        raise ValueError(f"{what}: n_embd = {wte.shape[1]}; the HIP decoder implements n_embd = 768 (12 heads of 64) only")
    head = sd.pop("lm_head.weight", None)
    if head is not None and (head.shape != wte.shape or not np.array_equal(head, wte)):
        raise ValueError(f"{what}: lm_head.weight is not tied to transformer.wte.weight; the HIP decoder implements the tied head only")
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in sd.items()}


# ---- the fine stage (csrc/fine.hip) -----------------------------------------------------------------------------------------------
FINE_TABLE_ROWS, FINE_CODE_BOOKS, FINE_HEADS = 1056, 8, 7
_FINE_LINEARS = ("attn.c_attn", "attn.c_proj", "mlp.c_fc", "mlp.c_proj")
# HF's BarkFineModel names -> bark's model_fine.py names, the canonical ones
_FINE_HF_NAMES = (("input_embeds_layers.", "transformer.wtes."), ("position_embeds_layer.", "transformer.wpe."), ("layernorm_final.", "transformer.ln_f."),
                  ("layers.", "transformer.h."))
_FINE_HF_PARTS = ((".layernorm_1.", ".ln_1."), (".layernorm_2.", ".ln_2."), (".attn.att_proj.", ".attn.c_attn."), (".attn.out_proj.", ".attn.c_proj."),
                  (".mlp.in_proj.", ".mlp.c_fc."), (".mlp.out_proj.", ".mlp.c_proj."))


def synth_fine_weights(n_layer: int = 12, hidden: int = 1024, block: int = 1024, seed: int = 0, family: str = "uniform", bias: bool = False) -> Dict[str, np.ndarray]:
    """Seeded synthetic weights of the fine stage under bark's names. ``"uniform"``: every matrix N(0, 0.02), the two ``c_proj`` at 0.02 / sqrt(2 n_layer);
    ``"peaky"``: the same with the heads at std 0.16, so that the logits spread over tens of units. LayerNorm gains are drawn from [0.8, 1.2] and
    LayerNorm biases from [-0.1, 0.1] (nonzero), so that a kernel that dropped either would not pass; ``bias=True`` adds N(0, 0.02) biases to the four
    linears of every block. The heads are not tied to the tables."""
    if family not in GPT_FAMILIES:
        raise ValueError(f"weight family {family!r}: one of {GPT_FAMILIES}")
    if hidden not in (768, 1024):
        raise ValueError(f"hidden = {hidden}: the fine stage is built for 768 or 1024")
    E, F = hidden, 4 * hidden
    proj_std = 0.02 / float(np.sqrt(2.0 * n_layer))
    jobs = [(f"transformer.wtes.{i}.weight", (FINE_TABLE_ROWS, E), 0.02) for i in range(FINE_CODE_BOOKS)]
    jobs += [("transformer.wpe.weight", (block, E), 0.02)]
    jobs += [(f"lm_heads.{j}.weight", (FINE_TABLE_ROWS, E), 0.16 if family == "peaky" else 0.02) for j in range(FINE_HEADS)]
    for i in range(n_layer):
        p = f"transformer.h.{i}"
        shapes = {"attn.c_attn": ((3 * E, E), 0.02), "attn.c_proj": ((E, E), proj_std), "mlp.c_fc": ((F, E), 0.02), "mlp.c_proj": ((E, F), proj_std)}
        for lin in _FINE_LINEARS:
            shape, std = shapes[lin]
            jobs.append((f"{p}.{lin}.weight", shape, std))
            if bias:
                jobs.append((f"{p}.{lin}.bias", (shape[0],), 0.02))
    w = _run_jobs([(name, (lambda name=name, shape=shape, std=std: prng.irwin_hall("fine." + name, shape, std, seed))) for name, shape, std in jobs])
    for name in [f"transformer.h.{i}.ln_{j}" for i in range(n_layer) for j in (1, 2)] + ["transformer.ln_f"]:
        w[name + ".weight"] = prng.uniform("fine." + name + ".weight", (E,), 0.8, 1.2, seed)
        b = prng.uniform("fine." + name + ".bias", (E,), 0.02, 0.1, seed)
        w[name + ".bias"] = b * np.where(prng.uniform01("fine." + name + ".sign", E, seed) < 0.5, np.float32(-1), np.float32(1))
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def read_fine_checkpoint(path) -> Dict[str, np.ndarray]:
    """A fine-stage checkpoint as the tensors ``at_fine_finalize`` takes: ``torch.load(path)``, the state dict itself or nested under ``["model"]``,
    under bark's names or HF's (``fine_tensors_from_state_dict``)."""
    import torch
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(ckpt, dict) and isinstance(ckpt.get("model"), dict):
        ckpt = ckpt["model"]
    if not isinstance(ckpt, dict):
        raise ValueError(f"{path}: not a fine-stage checkpoint (a state dict, or a dict with a 'model' state dict, is expected)")
    return fine_tensors_from_state_dict(ckpt, what=str(path))


def fine_tensors_from_state_dict(sd, what: str = "state dict") -> Dict[str, np.ndarray]:
    """{bark name: float32 array} from a state dict under bark's names (``transformer.wtes.{i}.weight``, ...) or HF's (``input_embeds_layers.{i}.weight``,
    ...), with an optional ``_orig_mod.`` prefix. Refused with ``ValueError``: a missing table, head or LayerNorm bias, a width other than 768 / 1024, a
    block that is no multiple of 128 in [128, 1024], linear biases on some linears only."""
    out: Dict[str, np.ndarray] = {}
    for k, v in sd.items():
        for pre in ("_orig_mod.", "fine_acoustics."):
            if k.startswith(pre):
                k = k[len(pre):]
        if k.endswith(".attn.bias"):      # a mask buffer, not a parameter
            continue
        for hf, ours in _FINE_HF_NAMES:
            if k.startswith(hf):
                k = ours + k[len(hf):]
                break
        for hf, ours in _FINE_HF_PARTS:
            k = k.replace(hf, ours)
        out[k] = np.ascontiguousarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else np.asarray(v, dtype=np.float32), dtype=np.float32)
    wpe = out.get("transformer.wpe.weight")
    if wpe is None or wpe.ndim != 2:
        raise ValueError(f"{what}: transformer.wpe.weight is missing")
    W, E = wpe.shape
    if E not in (768, 1024):
        raise ValueError(f"{what}: n_embd = {E}; the HIP fine stage implements 768 or 1024 (heads of 64)")
    if W % 128 or not 128 <= W <= 1024:
        raise ValueError(f"{what}: block size {W}; the HIP fine stage implements multiples of 128 from 128 to 1024")
    n_layer = 0
    while f"transformer.h.{n_layer}.ln_1.weight" in out:
        n_layer += 1
    if n_layer < 1:
        raise ValueError(f"{what}: no transformer block (transformer.h.0.ln_1.weight is missing)")
    need = {f"transformer.wtes.{i}.weight": (FINE_TABLE_ROWS, E) for i in range(FINE_CODE_BOOKS)}
    need.update({f"lm_heads.{j}.weight": (FINE_TABLE_ROWS, E) for j in range(FINE_HEADS)})
    need.update({"transformer.ln_f.weight": (E,), "transformer.ln_f.bias": (E,)})
    lin_shapes = {"attn.c_attn": (3 * E, E), "attn.c_proj": (E, E), "mlp.c_fc": (4 * E, E), "mlp.c_proj": (E, 4 * E)}
    biases = [f"transformer.h.{i}.{lin}.bias" for i in range(n_layer) for lin in _FINE_LINEARS]
    have = [b for b in biases if b in out]
    if have and len(have) != len(biases):
        missing = next(b for b in biases if b not in out)
        raise ValueError(f"{what}: mixed biases: {have[0]} is there and {missing} is not; the linears carry a bias in every block or in none")
    for i in range(n_layer):
        p = f"transformer.h.{i}"
        for ln in ("ln_1", "ln_2"):
            need[f"{p}.{ln}.weight"] = need[f"{p}.{ln}.bias"] = (E,)
        for lin, shape in lin_shapes.items():
            need[f"{p}.{lin}.weight"] = shape
            if have:
                need[f"{p}.{lin}.bias"] = (shape[0],)
    for name, shape in need.items():
        if name not in out:
            raise ValueError(f"{what}: {name} is missing")
        if tuple(out[name].shape) != shape:
            raise ValueError(f"{what}: {name} has shape {tuple(out[name].shape)}, expected {shape}")
    return {k: out[k] for k in need} | {"transformer.wpe.weight": wpe}


def read_hf_state_dict(model_dir: str, strip_prefixes=()) -> Dict[str, np.ndarray]:
    """A HF ``save_pretrained`` directory -> {name: float32 array}. Understands ``model.safetensors``, the sharded form
    (``model.safetensors.index.json`` + ``model-0000i-of-0000n.safetensors``) and the legacy ``pytorch_model.bin`` (+ its sharded index).
    Task-head prefixes such as ``"wav2vec2_bert."`` / ``"hubert."`` are removed."""
    import json
    import os
    sd: Dict[str, np.ndarray] = {}

    def add_safetensors(path):
        from safetensors import safe_open
        with safe_open(path, framework="pt", device="cpu") as f:      # "pt": also reads bf16 / fp16 checkpoints
            for k in f.keys():
                sd[k] = f.get_tensor(k).float().numpy()

    def add_bin(path):
        import torch
        for k, v in torch.load(path, map_location="cpu", weights_only=True).items():
            sd[k] = v.float().numpy()

    st, st_idx = os.path.join(model_dir, "model.safetensors"), os.path.join(model_dir, "model.safetensors.index.json")
    pt, pt_idx = os.path.join(model_dir, "pytorch_model.bin"), os.path.join(model_dir, "pytorch_model.bin.index.json")
    if os.path.exists(st):
        add_safetensors(st)
    elif os.path.exists(st_idx):
        with open(st_idx) as fh:
            for shard in sorted(set(json.load(fh)["weight_map"].values())):
                add_safetensors(os.path.join(model_dir, shard))
    elif os.path.exists(pt):
        add_bin(pt)
    elif os.path.exists(pt_idx):
        with open(pt_idx) as fh:
            for shard in sorted(set(json.load(fh)["weight_map"].values())):
                add_bin(os.path.join(model_dir, shard))
    else:
        raise FileNotFoundError(f"{model_dir}: no model.safetensors / model.safetensors.index.json / pytorch_model.bin")
    out = {}
    for k, v in sd.items():
        for pre in strip_prefixes:
            if k.startswith(pre):
                k = k[len(pre):]
                break
        out[k] = v
    return out


def check_hf_config(model_dir: str, expected: Dict[str, object], what: str) -> Optional[dict]:
    """If the directory has a config.json, the architecture fields the HIP kernels are built for must match; returns the config."""
    import json
    import os
    path = os.path.join(model_dir, "config.json")
    if not os.path.exists(path):
        return None
    with open(path) as fh:
        cfg = json.load(fh)
    bad = {k: (cfg.get(k), v) for k, v in expected.items() if k in cfg and cfg[k] != v}
    if bad:
        raise ValueError(f"{what}: {path} describes a different architecture than the kernels implement: "
                         + ", ".join(f"{k}={got!r} (need {want!r})" for k, (got, want) in bad.items()))
    return cfg


def missing_tensors(model: str, n: int, with_extras: bool, have: Dict[str, np.ndarray]):
    """Names (or shape mismatches) that the library's finalize() for `model` needs and `have` does not provide."""
    from . import _cabi
    out = []
    for name, shape in _cabi.required_tensors(model, n, with_extras).items():
        if name not in have:
            out.append(name)
        elif tuple(have[name].shape) != shape:
            out.append(f"{name}: shape {tuple(have[name].shape)} != {shape}")
    return out
