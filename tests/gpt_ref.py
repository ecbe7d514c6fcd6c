"""CPU twin of the semantic-to-acoustic GPT (audiotoken_amd/csrc/gpt.hip), written from the model's description: token embedding tied to the head, learned
positions, pre-LN blocks with gain-only LayerNorm (eps 1e-5), bias-free linears, 12 heads of 64, causal attention scaled by 1/8, an erf-GELU MLP, a final
LayerNorm. ``forward`` recomputes the whole sequence (no cache); ``sample`` follows the sampling rule literally."""
import math

import numpy as np
import torch

E, HEADS, HD = 768, 12, 64


def _ln(x, g):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g


def causal_attention(q, k, v):
    """q, k, v [heads, T, 64] -> [heads, T, 64]: softmax over keys j <= i of q_i . k_j / 8."""
    T = q.shape[-2]
    s = (q @ k.transpose(-1, -2)) * 0.125
    s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu(1), float("-inf"))
    return torch.softmax(s, dim=-1) @ v


def n_layers(w):
    n = 0
    while f"transformer.h.{n}.ln_1.weight" in w:
        n += 1
    return n


def forward(w, ids, dtype=torch.float64, positions=None):
    """Logits [len(positions) or T, V] of the sequence ``ids`` (int, [T]) in ``dtype``; ``positions``: the rows the head is applied to (default all)."""
    W = lambda name: torch.as_tensor(w[name]).to(dtype)
    ids = torch.as_tensor(np.asarray(ids), dtype=torch.int64)
    T = ids.numel()
    x = W("transformer.wte.weight")[ids] + W("transformer.wpe.weight")[:T]
    for i in range(n_layers(w)):
        p = f"transformer.h.{i}"
        qkv = _ln(x, W(p + ".ln_1.weight")) @ W(p + ".attn.c_attn.weight").t()
        q, k, v = (t.reshape(T, HEADS, HD).transpose(0, 1) for t in qkv.split(E, dim=-1))
        ctx = causal_attention(q, k, v).transpose(0, 1).reshape(T, E)
        x = x + ctx @ W(p + ".attn.c_proj.weight").t()
        h = _ln(x, W(p + ".ln_2.weight")) @ W(p + ".mlp.c_fc.weight").t()
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = x + h @ W(p + ".mlp.c_proj.weight").t()
    x = _ln(x, W("transformer.ln_f.weight"))
    if positions is not None:
        x = x[torch.as_tensor(positions, dtype=torch.int64)]
    return x @ W("transformer.wte.weight").t()


def kept_values(logits_f32, temperature, top_k, allow=None):
    """Steps 1 to 3 of the sampling rule: (kept ids ascending, their tempered float32 values). The division in fp32."""
    z = np.asarray(logits_f32, dtype=np.float32)
    V = z.shape[0]
    zt = (z / np.float32(temperature)).astype(np.float32)
    if allow is not None:
        ids = np.arange(V)
        ok = ((ids >= allow[0]) & (ids < allow[1])) | ((ids >= allow[2]) & (ids < allow[3]))
        zt = np.where(ok, zt, np.float32(-np.inf)).astype(np.float32)
    k = min(int(top_k), V)
    v = np.partition(zt, V - k)[V - k]          # the k-th largest
    kept = np.nonzero(zt >= v)[0]               # ascending ids; ties at the threshold stay
    return kept, zt[kept]


def kept_weights(logits_f32, temperature, top_k, allow=None):
    """Steps 1 to 4: (kept ids ascending, their float64 weights normalised to sum 1): what a softmax over the masked logits gives the kept ids."""
    kept, zk = kept_values(logits_f32, temperature, top_k, allow)
    p = np.exp(zk.astype(np.float64) - np.float64(zk.max()))
    return kept, p / p.sum()


def sample(logits_f32, temperature, top_k, u, allow=None):
    """The sampling rule on one float32 logit vector: (token, dist, kept). Step 1 (the division) in fp32, the rest in float64. ``allow``: None or
    (lo0, hi0, lo1, hi1), two half-open id ranges. ``dist`` is the distance from ``u`` to the nearest boundary between two kept ids in the kept set's normalised CDF."""
    kept, zk = kept_values(logits_f32, temperature, top_k, allow)
    z64 = zk.astype(np.float64)
    p = np.exp(z64 - z64.max())
    cdf = np.cumsum(p)
    S = cdf[-1]
    target = np.float64(np.float32(u)) * S
    over = np.nonzero(cdf > target)[0]
    token = int(kept[over[0]]) if over.size else int(kept[z64 > -np.inf][-1])   # the fallback: the highest kept id that is not -inf
    # the boundaries between two kept ids; the CDF's end (1) decides nothing: past it the rule takes the highest kept id that is not -inf, the id just below it too
    dist = float(np.abs(cdf[:-1] / S - np.float64(np.float32(u))).min()) if kept.size > 1 else float("inf")
    return token, dist, int(kept.size)
