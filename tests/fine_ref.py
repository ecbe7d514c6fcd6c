"""CPU twin of the fine stage (audiotoken_amd/csrc/fine.hip), written from the model's description: eight embedding tables summed up to the code book being
predicted, learned positions, pre-LN blocks (LayerNorm with gain and bias, eps 1e-5; linears with or without bias; heads of 64; attention over the whole
window with no mask, scaled by 1/8; an erf-GELU MLP), a final LayerNorm, seven heads of which head ``c - 1`` predicts code book ``c``. ``forward`` takes
one buffer or a batch of them; ``fine_windows`` is the window schedule, ``generate`` the loop, ``sample`` the sampling rule taken literally."""
import math

import numpy as np
import torch

HD = 64
VOCAB = 1024          # ids a head may produce; 1024 itself marks a cell that holds nothing yet
N_CODES, N_COARSE = 8, 2
# The device's running sum of id i: the lane's own ids up to i (at most 15 additions), the 6 levels of the shuffle scan over the lanes' totals and the
# addition of the two: at most 22 roundings of partial sums <= S, and one more in u * S: 23 * 2^-24 of S. Each p_i = expf(zt_i - m) carries 2 ulp of
# expf (2^-22, in the sum and in S alike) and the rounding of zt_i - m: a relative 2^-24 |zt_i - m| of p_i, over the ids at most 2^-24 E_p[m - zt] <=
# 2^-24 ln 1024 < 7 * 2^-24 of S (the mean of m - zt under the softmax is its entropy minus ln(S), at most ln 1024). Both sides of the comparison: twice.
WINDOW = 2.0 * ((23 + 7) * 2.0 ** -24 + 2.0 ** -22)


def _ln(x, g, b):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) * g + b


def n_layers(w):
    n = 0
    while f"transformer.h.{n}.ln_1.weight" in w:
        n += 1
    return n


def attention(q, k, v, drop_last_keys=0):
    """q, k, v [..., heads, T, 64] -> the same shape: softmax over every key of q_i . k_j / 8. ``drop_last_keys``: a mutant that does not see the last
    that many keys (what a kernel that lost its last key tile computes)."""
    if drop_last_keys:
        k, v = k[..., :-drop_last_keys, :], v[..., :-drop_last_keys, :]
    return torch.softmax((q @ k.transpose(-1, -2)) * 0.125, dim=-1) @ v


def forward(w, buf, c, dtype=torch.float64, positions=None, drop_last_keys=0):
    """Logits ``[..., len(positions) or W, 1024]`` for code book ``c`` (2 to 7) of the buffer(s) ``buf`` (int ``[..., W, 8]``, ids in [0, 1024])."""
    Wt = lambda name: torch.as_tensor(w[name]).to(dtype)
    bias = lambda name: Wt(name) if name in w else 0.0
    buf = torch.as_tensor(np.asarray(buf), dtype=torch.int64)
    T = buf.shape[-2]
    E = w["transformer.wpe.weight"].shape[1]
    heads = E // HD
    x = Wt("transformer.wtes.0.weight")[buf[..., 0]]
    for i in range(1, c + 1):
        x = x + Wt(f"transformer.wtes.{i}.weight")[buf[..., i]]
    x = x + Wt("transformer.wpe.weight")[:T]
    lead = x.shape[:-2]
    for i in range(n_layers(w)):
        p = f"transformer.h.{i}"
        qkv = _ln(x, Wt(p + ".ln_1.weight"), Wt(p + ".ln_1.bias")) @ Wt(p + ".attn.c_attn.weight").t() + bias(p + ".attn.c_attn.bias")
        q, k, v = (t.reshape(*lead, T, heads, HD).transpose(-2, -3) for t in qkv.split(E, dim=-1))
        ctx = attention(q, k, v, drop_last_keys).transpose(-2, -3).reshape(*lead, T, E)
        x = x + ctx @ Wt(p + ".attn.c_proj.weight").t() + bias(p + ".attn.c_proj.bias")
        h = _ln(x, Wt(p + ".ln_2.weight"), Wt(p + ".ln_2.bias")) @ Wt(p + ".mlp.c_fc.weight").t() + bias(p + ".mlp.c_fc.bias")
        h = 0.5 * h * (1.0 + torch.erf(h / math.sqrt(2.0)))
        x = x + h @ Wt(p + ".mlp.c_proj.weight").t() + bias(p + ".mlp.c_proj.bias")
    x = _ln(x, Wt("transformer.ln_f.weight"), Wt("transformer.ln_f.bias"))
    if positions is not None:
        x = x[..., torch.as_tensor(positions, dtype=torch.int64), :]
    return x @ Wt(f"lm_heads.{c - 1}.weight")[:VOCAB].t()


def fine_windows(T, W):
    """[(start, fill)] of a row of ``T`` frames at block ``W``, hop ``H = W / 2``: ``n = max(0, ceil((T - W) / H)) + 1`` windows over a work array of
    ``L = max(T, W)`` cells, ``start = min(k H, L - W)``, ``fill = min(k H, L - H)``."""
    H, L = W // 2, max(T, W)
    n = max(0, math.ceil((T - W) / H)) + 1
    return [(min(k * H, L - W), min(k * H, L - H)) for k in range(n)]


def sample_many(logits_f32, temperature, u):
    """The sampling rule on float32 logit vectors ``[N, 1024]`` with draws ``u [N]``: (tokens ``[N]``, dists ``[N]``). The division in fp32, the rest in
    float64. ``temperature=None``: the argmax, the lowest id among equals (``dist`` is then infinite: no draw decides anything). ``dist``: the distance from
    ``u`` to the nearest boundary between two ids in the normalised CDF."""
    z = np.asarray(logits_f32, dtype=np.float32).reshape(-1, VOCAB)
    if temperature is None:
        return np.argmax(z, axis=-1), np.full(z.shape[0], np.inf)
    zt = (z / np.float32(temperature)).astype(np.float32).astype(np.float64)
    p = np.exp(zt - zt.max(-1, keepdims=True))
    cdf = np.cumsum(p, axis=-1)
    S = cdf[:, -1:]
    u = np.asarray(u, dtype=np.float32).astype(np.float64).reshape(-1, 1)
    over = cdf > u * S
    last = VOCAB - 1 - np.argmax((p > 0)[:, ::-1], axis=-1)          # the fallback: the highest id of nonzero weight
    tokens = np.where(over.any(-1), np.argmax(over, axis=-1), last)
    return tokens, np.abs(cdf[:, :-1] / S - u).min(-1)


def sample(logits_f32, temperature, u):
    """``sample_many`` on one vector: (token, dist)."""
    tok, dist = sample_many(np.asarray(logits_f32)[None], temperature, None if temperature is None else [u])
    return int(tok[0]), float(dist[0])


def work_array(coarse, W):
    """The row's work array ``[max(T, W), 8]``: 1024 everywhere but the coarse codes."""
    coarse = np.asarray(coarse)
    T = coarse.shape[1]
    work = np.full((max(T, W), N_CODES), VOCAB, dtype=np.int64)
    work[:T, :N_COARSE] = coarse.T
    return work


def generate(w, coarse, temperature, uniforms=None, dtype=torch.float32):
    """The loop on one row ``coarse`` (int ``[2, T]``) with the twin's own forward in ``dtype``: (codes ``[8, T]``, every draw's distance to the nearest
    CDF boundary). ``uniforms``: float32 ``[n, 6, W]``."""
    W = w["transformer.wpe.weight"].shape[0]
    T = np.asarray(coarse).shape[1]
    work = work_array(coarse, W)
    dists = []
    for k, (start, fill) in enumerate(fine_windows(T, W)):
        rel = fill - start
        for c in range(N_COARSE, N_CODES):
            logits = forward(w, work[start:start + W], c, dtype, positions=list(range(rel, W))).float().numpy()
            tok, dist = sample_many(logits, temperature, None if temperature is None else uniforms[k, c - N_COARSE, rel:])
            dists.append(dist)
            work[start + rel:start + W, c] = tok
    return work[:T].T.copy(), np.concatenate(dists)
