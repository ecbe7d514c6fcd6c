"""What the CPU and the GPU tests of the semantic-to-audio stream share: the push splittings, the brute-force statement of the rule,
and the two twins (tests/gpt_ref.py, tests/fine_ref.py) driven by the stream's schedule."""
import numpy as np
import torch

from tests import fine_ref
from tests import gpt_ref as R
from tests import long_form_cases as K


def splittings(N, S, H, seed=0):
    """{name: ids per push} for a source of N ids: all at once, one id at a time, a fixed-seed random split, and splits whose pushes end exactly at
    ``k H + S`` and at ``k H + S + 1`` for every k that fits."""
    rng = np.random.default_rng(1000 * seed + N)
    cuts = sorted(set(rng.integers(1, N, size=max(1, N // 5)).tolist())) if N > 1 else []
    out = {"all": [N], "ones": [1] * N, "random": np.diff([0] + cuts + [N]).tolist()}
    for name, extra in (("at_window", 0), ("past_window", 1)):
        edges = [k * H + S + extra for k in range(N) if k * H + S + extra < N]
        out[name] = np.diff([0] + edges + [N]).tolist()
    assert all(sum(p) == N and min(p) >= 1 for p in out.values())
    return out


def write_sets(windows, T, W):
    """Per fine window ``(start, fill)``: the row's frames it writes (its predicted positions that are real frames)."""
    return [range(fill, min(start + W, T)) for start, fill in windows]


def stream_twin(w_gpt, cfg, w_fine, src, pushes, u_row, fine_u, max_new=K.MAX_NEW, S=K.S, H=K.H, r=K.r, block=K.BLOCK, temperature=K.TEMPERATURE, top_k=K.TOP_K,
                fine_temperature=0.5):
    """The two twins driven push by push: a GPT window runs when its inputs exist (decided from the ids pushed so far alone), its ids are handed over as frames, a fine window runs when its frames exist, and frames are emitted when final. Returns (stream of raw ids,
    finish, codes [8, T] in emission order, the events). The rule is restated here by hand, not taken from ``stream_schedule``."""
    W = w_fine["transformer.wpe.weight"].shape[0]
    src = np.asarray(src)
    stream, finish, pushed, k_next = [], None, 0, 0
    work = np.zeros((0, fine_ref.N_CODES), dtype=np.int64)
    emitted, n_fine, events = [], 0, []
    for i, n_new in enumerate(list(pushes) + [0]):
        final = i == len(pushes)
        pushed += n_new
        seen = src[:pushed]                                     # all the stream may look at
        made, ks = 0, []
        while not final and pushed > k_next * H + S:            # one id past the window exists: it is not the final one
            ks.append(k_next)
            k_next += 1
        if final:
            ks.append(k_next)                                   # the one remaining window
        for k in ks:
            carry = r * (S - H) if k else 0
            n_src = len(seen) - k * H if final else S
            prompt, base = K.window_prompt(cfg, seen, stream, (k * H, n_src, carry, None), r)
            assert base == len(stream)
            allow = K.allow_of(cfg, final)
            budget = min(max_new, block - len(prompt)) if final else r * S - carry
            seq = prompt
            for s in range(budget):
                logits = R.forward(w_gpt, seq, torch.float32, positions=[len(seq) - 1])[0].numpy()
                tok, _, _ = R.sample(logits, temperature, top_k, u_row[base + s], allow[s % 2])
                if final and tok == cfg.STOP_TOKEN:
                    finish = "stop"
                    break
                stream.append(tok)
                seq = np.append(seq, tok)
                made += 1
            if final and finish is None:
                finish = "max_new_tokens" if budget == max_new else "block_size"
        # the hand-over: whole frames only
        T = len(stream) // 2
        for t in range(work.shape[0], T):
            cell = np.full((1, fine_ref.N_CODES), fine_ref.VOCAB, dtype=np.int64)
            cell[0, 0] = stream[2 * t] - cfg.ACOUSTIC_OFFSET
            cell[0, 1] = stream[2 * t + 1] - cfg.ACOUSTIC_OFFSET - cfg.codebook_size
            work = np.concatenate([work, cell])
        # the fine windows whose frames exist now, and at the flush the row's last
        todo = []
        while n_fine * (W // 2) + W <= T:
            todo.append((n_fine * (W // 2), 0))
            n_fine += 1
        if final:
            if T < W:
                work = np.concatenate([work, np.full((W - T, fine_ref.N_CODES), fine_ref.VOCAB, dtype=np.int64)])
                todo.append((0, 0))
            elif (T - W) % (W // 2):
                todo.append((T - W, n_fine * (W // 2) - (T - W)))
        for start, rel in todo:
            j = start // (W // 2) if rel == 0 else n_fine
            for c in range(fine_ref.N_COARSE, fine_ref.N_CODES):
                logits = fine_ref.forward(w_fine, work[start:start + W], c, torch.float32, positions=list(range(rel, W))).float().numpy()
                tok, _ = fine_ref.sample_many(logits, fine_temperature, fine_u[j, c - fine_ref.N_COARSE, rel:])
                work[start + rel:start + W, c] = tok
        upto = T if final else n_fine * (W // 2)
        emitted.extend(work[t].copy() for t in range(len(emitted), upto))
        events.append({"made": made, "frames": T, "fine": todo, "emitted": upto})
    return np.asarray(stream, dtype=np.int64), finish, np.asarray(emitted).T.copy(), events
