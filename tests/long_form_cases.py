"""What the CPU and the GPU tests of the long form share: the small token space, the inputs, the window prompts rebuilt from a stream,
and the twin's own chained generation (tests/gpt_ref.py, uncached)."""
import numpy as np
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.configs import HubertDecoderConfig
from audiotoken_amd.semantic_decoder import acoustic_windows, seeded_uniforms

from tests import gpt_ref as R

# A token space of 2048 ids declared through the config's own fields: semantic ids [64, 320), code book 0 [512, 1024), code book 1 [1024, 1536)
CFG = HubertDecoderConfig(TEXT_VOCAB_SIZE=64, SEMANTIC_VOCAB_SIZE=256, ACOUSTIC_VOCAB_SIZE=1024, SEMANTIC_OFFSET=64, ACOUSTIC_OFFSET=512, INFER_TOKEN=1600,
                          STOP_TOKEN=1601, VOCAB_SIZE=2048, max_source_tokens=8, codebook_size=512, weights=None)
CFG_PRODUCT = HubertDecoderConfig(TEXT_VOCAB_SIZE=64, SEMANTIC_VOCAB_SIZE=256, ACOUSTIC_VOCAB_SIZE=1024, SEMANTIC_OFFSET=64, ACOUSTIC_OFFSET=512,
                                  INFER_TOKEN=1600, STOP_TOKEN=1601, VOCAB_SIZE=2048, max_source_tokens=250, codebook_size=512, weights=None)
V = 2048
S, H, r, BLOCK = 8, 4, 3, 64
SEED = 2024
TEMPERATURE, TOP_K = 0.8, 100
MAX_NEW = 10          # the final window's budget in the small cases
FAMILIES = ("uniform", "peaky")
LENGTHS = [1, S - 1, S, S + 1, S + H, S + H + 1, 2 * S + 3]
MIXED_ROWS = [1, S, S + 1, 2 * S + 3]

_weights = {}


def weights(family, block=BLOCK):
    if (family, block) not in _weights:
        _weights[(family, block)] = W.synth_gpt_weights(n_layer=2, vocab=V, block=block, seed=0, family=family)
    return _weights[(family, block)]


def source(N, seed=0, cfg=CFG):
    return np.random.default_rng(104729 * seed + N).integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=N).astype(np.int64)


def allow_of(cfg, final):
    a, n = cfg.ACOUSTIC_OFFSET, cfg.codebook_size
    even = [a, a + n, cfg.STOP_TOKEN, cfg.STOP_TOKEN + 1] if final else [a, a + n, 0, 0]
    return [even, [a + n, a + 2 * n, 0, 0]]


def window_prompt(cfg, src, stream, window, r=r):
    """The prompt of one window ``(source_start, source_len, carry, _)``: source ids + the offset, INFER, the ``carry`` ids of ``stream`` (raw model ids)
    from position ``r * source_start`` on. Returns (prompt, the stream position of the window's first new id)."""
    start, n_src, carry, _ = window
    prompt = np.concatenate([np.asarray(src[start:start + n_src]) + cfg.SEMANTIC_OFFSET, [cfg.INFER_TOKEN], np.asarray(stream[r * start:r * start + carry])])
    return prompt.astype(np.int64), r * start + carry


def capacity(N, max_new, S=S, H=H, r=r, block=BLOCK):
    """Stream positions the row of a source of N ids can reach."""
    start, n_src, carry, _ = acoustic_windows(N, S, H, r, block)[-1]
    return r * start + carry + min(max_new, block - (n_src + 1 + carry))


def draws(rows, max_new, seed=SEED, **geometry):
    """float32 [B, L]: one draw per row and stream position, ``max_new`` wider than the longest row needs (so that a by-hand final window, which takes
    ``max_new`` draws whatever its budget, finds them)."""
    return seeded_uniforms(seed, len(rows), max(capacity(N, max_new, **geometry) for N in rows) + max_new)


def twin_chain(w, cfg, src, u_row, max_new=MAX_NEW, S=S, H=H, r=r, block=BLOCK, temperature=TEMPERATURE, top_k=TOP_K):
    """The schedule run on the twin alone, every step an uncached float32 forward. Returns (stream of raw ids, finish, [(stream position, dist, kept)])."""
    plan = acoustic_windows(len(src), S, H, r, block)
    stream, trace, finish = [], [], None
    for k, win in enumerate(plan):
        final = k == len(plan) - 1
        prompt, base = window_prompt(cfg, src, stream, win, r)
        assert base == len(stream), "a window starts where the one before ended"
        allow = allow_of(cfg, final)
        budget = min(max_new, block - len(prompt)) if final else win[3]
        seq = prompt
        for s in range(budget):
            logits = R.forward(w, seq, torch.float32, positions=[len(seq) - 1])[0].numpy()
            tok, dist, kept = R.sample(logits, temperature, top_k, u_row[base + s], allow[s % 2])
            trace.append((base + s, dist, kept))
            if final and tok == cfg.STOP_TOKEN:
                finish = "stop"
                break
            stream.append(tok)
            seq = np.append(seq, tok)
        if final and finish is None:
            finish = "max_new_tokens" if budget == max_new else "block_size"
    return np.asarray(stream, dtype=np.int64), finish, trace
