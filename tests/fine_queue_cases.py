"""What tests/test_fine_queue_gpu.py runs and tests/test_fine_queue_cpu.py qualifies without a device: the rows, the per-row draws and the protocol of
the fine stage's window queue, in one place so that both files use the very same inputs. Models and weights are those of
tests/fine_cases.py."""
import numpy as np
import torch

from audiotoken_amd.fine_decoder import row_uniforms

from tests import fine_cases as K
from tests import fine_ref as R
from tests.parity import FLOAT_TOL

SEED = 4242   # the draws of every GPU test of the queue; the CPU file shows that the twin's own generation leaves them off the CDF boundaries


def mixed_lengths(W):
    """12 rows of 1 to 4 windows: odd sizes, sizes at and next to the schedule's edges."""
    H = W // 2
    return [W + 1, 5, 2 * W + 3, W, W + H + 1, H, 2 * W + H, W - 1, W + H, 2 * W, 1, 2 * W + 1]


MIXED_WINDOWS = [2, 1, 4, 1, 3, 1, 4, 1, 2, 3, 1, 4]


def single_slot_lengths(W):
    return [1, W // 2, W, W + 1, 2 * W + 3]


def row(i, T):
    """Row ``i`` of a case: its coarse codes depend on (i, T) alone."""
    return K.coarse_row(T, seed=i)


def draws(i, T, W, seed=SEED):
    """Row ``i``'s draws ``[n, 6, W]``: keyed by (seed, i), so a row keeps its draws wherever it stands in a call."""
    return row_uniforms(seed, i, len(R.fine_windows(T, W)), W)


def verify(w, W, rows, gen, uniforms, temperature, raw=None):
    """§18's protocol for ragged draws (``uniforms``: a list of per-row ``[n_b, 6, W]``), per row teacher-forced on the device's own ids: (a) the float64
    twin on the buffers the device saw bounds the logits by ``FLOAT_TOL``; (b) the device's id equals ``fine_ref.sample_many`` on the DEVICE's logits with
    that cell's draw, waived only inside ``fine_ref.WINDOW`` of a CDF boundary, for at most ``WAIVER_CAP`` of the test's draws and never on the argmax
    path; (c) the output equals the write-back rule; ``raw``: the whole ragged output buffer, which holds the rows back to back and nothing else.
    Returns (largest logit difference, waived, draws)."""
    waived = n_draws = 0
    worst = 0.0
    seen = {c: [] for c in range(2, 8)}
    for b, coarse in enumerate(rows):
        T = coarse.shape[1]
        sched = R.fine_windows(T, W)
        L, ids = gen.logits[b].numpy(), gen.window_ids[b].numpy()
        assert L.shape == (len(sched), 6, W, 1024) and ids.shape == (len(sched), 6, W)
        work = R.work_array(coarse, W)
        for k, (start, fill) in enumerate(sched):
            rel = fill - start
            assert bool((ids[k, :, :rel] == -1).all()) and bool(np.isnan(L[k, :, :rel]).all()), "nothing is written below rel"
            assert bool((ids[k, :, rel:] >= 0).all()) and bool((ids[k, :, rel:] < 1024).all())
            for c in range(2, 8):
                dev_logits = L[k, c - 2, rel:]
                seen[c].append((b, k, rel, work[start:start + W].copy(), dev_logits))
                u = None if temperature is None else uniforms[b][k, c - 2, rel:]
                tok, dist = R.sample_many(dev_logits, temperature, u)
                bad = np.nonzero(tok != ids[k, c - 2, rel:])[0]
                for t in bad:
                    assert temperature is not None, f"row {b} window {k} code book {c} position {rel + t}: the argmax has no waiver"
                    assert dist[t] < R.WINDOW, (f"row {b} window {k} code book {c} position {rel + t}: device id {ids[k, c - 2, rel + t]}, rule gives {tok[t]}, "
                                                f"{dist[t]:.3e} from a boundary (window {R.WINDOW:.3e})")
                waived += len(bad)
                n_draws += W - rel
                work[start + rel:start + W, c] = ids[k, c - 2, rel:]
        codes = gen.codes[b].numpy()
        assert codes.shape == (8, T) and gen.codes[b].dtype == torch.int64
        assert np.array_equal(codes[:2], coarse), "channels 0 and 1 are the input"
        assert np.array_equal(codes, work[:T].T), "the output is what the write-back rule makes of the ids"
    if raw is not None:
        assert np.array_equal(raw.numpy(), np.concatenate([g.numpy().reshape(-1) for g in gen.codes])), "the rows lie back to back, nothing is padded"
    for c, items in seen.items():
        for i in range(0, len(items), 32):
            chunk = items[i:i + 32]
            ref = R.forward(w, np.stack([it[3] for it in chunk]), c, torch.float64).numpy()
            for (b, k, rel, _, dev_logits), r in zip(chunk, ref):
                diff = float(np.abs(dev_logits.astype(np.float64) - r[rel:]).max())
                worst = max(worst, diff)
                assert diff <= FLOAT_TOL, f"row {b} window {k} code book {c}: logits differ from the float64 twin by {diff:.3e}"
    print(f"largest logit difference {worst:.3e}; waived {waived} of {n_draws} draws")
    assert waived <= K.WAIVER_CAP * n_draws
    return worst, waived, n_draws
