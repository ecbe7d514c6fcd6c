"""What the CPU and the GPU tests of the GPT's voice prompts share, on top of tests/long_form_cases.py: seeded prompts in its small token
space, the concatenated source and stream of a prompted row (prompt ids then source ids; the prompt's coarse ids then the row's result), on which the
prompt-free helpers (``window_prompt``, the protocol) apply unchanged, and the twin's own chained generation after a prompt."""
import numpy as np
import torch

from audiotoken_amd.semantic_decoder import acoustic_windows, seeded_uniforms
from audiotoken_amd.voice import VoicePrompt

from tests import gpt_ref as R
from tests import long_form_cases as K

PROMPTS = (2, 4)                      # P = 2 and P = S - H at (8, 4)
TOTALS = [K.S - 1, K.S, K.S + 1, K.S + K.H + 1, 2 * K.S + 3]   # P + N


def prompt(P, seed=0, cfg=K.CFG, rows=2):
    g = np.random.default_rng(7919 * seed + P)
    return VoicePrompt(g.integers(0, cfg.SEMANTIC_VOCAB_SIZE, size=P), g.integers(0, cfg.codebook_size, size=(rows, 3 * P // 2)), cfg.SEMANTIC_VOCAB_SIZE)


def given_stream(cfg, vp):
    """Stream positions [0, r P) of a prompted row as raw model ids: position p holds codes[p & 1][p >> 1] + the acoustic offset + (p & 1) code book sizes."""
    c = vp.codes[:2].numpy()
    p = np.arange(2 * c.shape[1])
    return c[p & 1, p >> 1] + cfg.ACOUSTIC_OFFSET + (p & 1) * cfg.codebook_size


def concatenated(vp, src):
    return np.asarray(src) if vp is None else np.concatenate([vp.semantic.numpy(), np.asarray(src)])


def result_capacity(P, N, max_new, S=K.S, H=K.H, r=K.r, block=K.BLOCK):
    start, n_src, carry, _ = acoustic_windows(N, S, H, r, block, P)[-1]
    return r * start + carry - r * P + min(max_new, block - (n_src + 1 + carry))


def draws(rows, max_new, seed=K.SEED, **geometry):
    """float32 [B, L] for rows of (P, N): one draw per RESULT position, ``max_new`` wider than the longest row needs."""
    return seeded_uniforms(seed, len(rows), max(result_capacity(P, N, max_new, **geometry) for P, N in rows) + max_new)


def twin_chain(w, cfg, vp, src, u_row, max_new=K.MAX_NEW, S=K.S, H=K.H, r=K.r, block=K.BLOCK, temperature=K.TEMPERATURE, top_k=K.TOP_K):
    """The prompted schedule on the twin alone, every step an uncached float32 forward. Returns (result as raw ids, finish, [(result position, dist, kept)])."""
    P = 0 if vp is None else len(vp)
    C = concatenated(vp, src)
    plan = acoustic_windows(len(src), S, H, r, block, P)
    stream = [] if vp is None else given_stream(cfg, vp).tolist()
    trace, finish = [], None
    for k, win in enumerate(plan):
        final = k == len(plan) - 1
        prompt_k, base = K.window_prompt(cfg, C, stream, win, r)
        assert base == len(stream), "a window starts where the one before ended (window 0: where the given ids end)"
        allow = K.allow_of(cfg, final)
        budget = min(max_new, block - len(prompt_k)) if final else win[3]
        seq = prompt_k
        for s in range(budget):
            logits = R.forward(w, seq, torch.float32, positions=[len(seq) - 1])[0].numpy()
            tok, dist, kept = R.sample(logits, temperature, top_k, u_row[base - r * P + s], allow[s % 2])
            trace.append((base - r * P + s, dist, kept))
            if final and tok == cfg.STOP_TOKEN:
                finish = "stop"
                break
            stream.append(tok)
            seq = np.append(seq, tok)
        if final and finish is None:
            finish = "max_new_tokens" if budget == max_new else "block_size"
    return np.asarray(stream[r * P:], dtype=np.int64), finish, trace
