"""CPU twin of the fine stage's history rule (``BarkFineModel.generate`` with ``history_prompt["fine_prompt"]``), on top of tests/fine_ref.py,
whose model, sampler and bounds it uses unchanged. A row of ``T`` frames continues a history of ``Th`` frames: the last ``h = min(H, Th)`` of them stand in
cells ``[0, h)`` of the work array in all 8 channels, the row's coarse codes in cells ``[h, h + T)``; the history is read and never written."""
import math

import numpy as np
import torch

from tests import fine_ref as R


def cells(Th, W):
    """h: the history cells of a row that continues ``Th`` frames (0: no history)."""
    return min(W // 2, Th)


def fine_windows(T, W, h):
    """[(start, fill)]: ``n = max(0, ceil((T - (W - h)) / H)) + 1`` windows over ``L = max(h + T, W)`` cells, ``start = min(k H, L - W)``,
    ``fill = min(h + k H, L - H)``."""
    H, L = W // 2, max(h + T, W)
    n = max(0, math.ceil((T - (W - h)) / H)) + 1
    return [(min(k * H, L - W), min(h + k * H, L - H)) for k in range(n)]


def brute_force_windows(T, W, h):
    """The same schedule found by walking the frames, with no closed form: a window starts every H cells, slides back to end at the array's end, and
    predicts every cell from its fill point on; windows are added until the cell after the last predicted one is past the row."""
    H, L = W // 2, max(h + T, W)
    out, k = [], 0
    while True:
        start = k * H
        while start + W > L:
            start -= 1
        fill = h + k * H
        while fill + H > L:
            fill -= 1
        out.append((start, fill))
        if start + W >= h + T:       # this window predicted through the row's last frame
            return out
        k += 1


def work_array(coarse, W, history=None):
    """``[max(h + T, W), 8]``: the history's last h frames, then the coarse codes, 1024 everywhere else; and h."""
    coarse = np.asarray(coarse)
    T = coarse.shape[1]
    h = 0 if history is None else cells(np.asarray(history).shape[1], W)
    work = np.full((max(h + T, W), R.N_CODES), R.VOCAB, dtype=np.int64)
    if h:
        work[:h] = np.asarray(history)[:, -h:].T
    work[h:h + T, :R.N_COARSE] = coarse.T
    return work, h


def generate(w, coarse, history, temperature, uniforms=None, dtype=torch.float32):
    """The loop on one row with the twin's own forward: (codes ``[8, T]``, every draw's distance to the nearest CDF boundary). ``uniforms``: float32
    ``[n, 6, W]``."""
    W = w["transformer.wpe.weight"].shape[0]
    T = np.asarray(coarse).shape[1]
    work, h = work_array(coarse, W, history)
    dists = []
    for k, (start, fill) in enumerate(fine_windows(T, W, h)):
        rel = fill - start
        for c in range(R.N_COARSE, R.N_CODES):
            logits = R.forward(w, work[start:start + W], c, dtype, positions=list(range(rel, W))).float().numpy()
            tok, dist = R.sample_many(logits, temperature, None if temperature is None else uniforms[k, c - R.N_COARSE, rel:])
            dists.append(dist)
            work[start + rel:start + W, c] = tok
    return work[h:h + T].T.copy(), np.concatenate(dists)
