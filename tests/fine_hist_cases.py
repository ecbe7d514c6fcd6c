"""What tests/test_fine_history_gpu.py runs and tests/test_fine_history_cpu.py qualifies without a device: the (Th, T) grid of the history golden
(tests/golden/make_golden_fine_history.py), the histories, and the draws, on the models and rows of tests/fine_cases.py."""
import numpy as np

from audiotoken_amd.fine_decoder import seeded_uniforms

from tests import fine_cases as K
from tests import fine_hist_ref as HR


def history_lengths(block):
    """Th: one frame, one short of the cap, the cap H = W / 2, and past it (only the last H frames count)."""
    H = block // 2
    return [1, H - 1, H, H + 5]


def row_lengths(block, h):
    """T: one frame, one short of a full first window, exactly full, the first row of two windows, and a row of three or four."""
    H = block // 2
    return [1, block - h - 1, block - h, block - h + 1, block + H + 1]


def grid(block):
    return [(Th, T) for Th in history_lengths(block) for T in row_lengths(block, HR.cells(Th, block))]


def history(Th, seed=0):
    """int64 [8, Th] with ids in [0, 1024)."""
    return np.random.default_rng(104729 * seed + 31 * Th + 5).integers(0, 1024, size=(8, Th))


def draws(rows, block, seed=K.SEED):
    """float32 [B, n_max, 6, W] for rows given as (T, h)."""
    n_max = max(len(HR.fine_windows(T, block, h)) for T, h in rows)
    return seeded_uniforms(seed, len(rows), n_max, block)


# The dropped-history case: model a, peaky, Th = H and T = H, so window 0 is exactly the history and the row, every key a real frame, and its first pass
# (code book 2) is known without a device. The CPU file shows that the twin without the history (the same row in cells [0, T)), and the twin with the
# history shifted by one frame, move the logits of the row's frames by more than 8 times the float bar; the GPU file compares exactly these logits.
DROPPED = dict(model="a", family="peaky", Th=64, T=64, seed=3)
