"""CPU twin of teacher-forced scoring (audiotoken_amd/csrc/gpt_score.hip), written from the rule's text: ``score`` is the row rule in
float64 on float32 logits, ``score_sequence`` the model (tests/gpt_ref.py, uncached) followed by the rule at every scored position, ``long_rows`` the long
form's rows built from DESIGN.md §19's description of a window, not from the package's code."""
import math

import numpy as np
import torch

from tests import gpt_ref as R

# |device logprob - score()| on the same fp32 logits (DESIGN.md §23 derives it from the kernel's order of additions). With u = 2^-24:
#   zt_t - m                      one rounding                                              u |d|
#   the arguments zt_i - m        one rounding each; exp turns it into a relative error of its term, and the weighted mean of |zt_i - m| under the
#                                 softmax is the entropy minus log S, at most ln V                                     u ln V
#   expf                          2 ulp                                                     4 u
#   S                             every term passes through at most ADD_DEPTH additions of non-negative numbers        ADD_DEPTH u
#   logf(S)                       2 ulp of a value in [0, ln V]                              4 u ln V
#   (zt_t - m) - logf(S)          one rounding                                              u (|d| + ln V)
# ADD_DEPTH: 2 (a lane's four weights, pairwise) + 16 (a lane's running sum over the at most 16 groups of 256 ids a wave owns at V = 65536) + 6 (the butterfly
# over 64 lanes) + 15 (16 waves in index order). ln 65536 < 11.1, so the constant part is (39 + 4 + 6 * 11.1) u < 110 u.
ADD_DEPTH = 39
BOUND_CONST = 110.0
U = 2.0 ** -24


def logprob_bound(d):
    """The derived bound for a target whose tempered logit lies ``d`` below the row's maximum."""
    return U * (2.0 * abs(float(d)) + BOUND_CONST)


def tempered(logits_f32, temperature, allow=None):
    """Steps 1 and 2: float32 ``z / T`` (one fp32 division), -inf outside the two half-open allow ranges."""
    z = np.asarray(logits_f32, dtype=np.float32)
    zt = (z / np.float32(temperature)).astype(np.float32)
    if allow is not None:
        ids = np.arange(z.shape[0])
        ok = ((ids >= allow[0]) & (ids < allow[1])) | ((ids >= allow[2]) & (ids < allow[3]))
        zt = np.where(ok, zt, np.float32(-np.inf)).astype(np.float32)
    return zt


def score(logits_f32, target, temperature=1.0, allow=None):
    """The row rule: ``(logprob float64, rank int)``. A target that is not allowed (or not an id) gets ``(-inf, V)``."""
    zt = tempered(logits_f32, temperature, allow)
    V = zt.shape[0]
    t = int(target)
    if not 0 <= t < V or (allow is not None and not (allow[0] <= t < allow[1] or allow[2] <= t < allow[3])):
        return -math.inf, V
    z64 = zt.astype(np.float64)
    m = z64.max()
    S = np.exp(z64 - m).sum()
    return float((z64[t] - m) - np.log(S)), int((zt > zt[t]).sum())


def score_sequence(w, ids, score_from, temperature=1.0, allow=None, dtype=torch.float64, at=lambda p: p - 1):
    """Every position p of ``ids`` from ``score_from`` on, scored against ``ids[p]`` on the model's logits at position p - 1, the allow set of a position
    being ``allow[(p - score_from) % 2]``: ``(logprob [n] float64, rank [n], logits [n, V] in dtype)``. The rule takes float32 logits, as the device has
    them: the float64 logits are rounded once. ``at``: which position's logits score p (the mutant checks replace it)."""
    ids = np.asarray(ids)
    positions = [at(p) for p in range(score_from, len(ids))]
    logits = R.forward(w, ids, dtype, positions=positions).numpy()
    lp, rank = [], []
    for j, p in enumerate(range(score_from, len(ids))):
        a, b = score(logits[j].astype(np.float32), ids[p], temperature, None if allow is None else allow[j % 2])
        lp.append(a)
        rank.append(b)
    return np.asarray(lp, dtype=np.float64), np.asarray(rank, dtype=np.int64), logits


def long_rows(src, stream, S, H, r, semantic_offset, infer_token, stop_token=None):
    """The rows the long form scores for one source of ``len(src)`` ids whose whole stream is given (model ids). DESIGN.md §19: a source of N <= S ids is
    one window; a longer one has ceil((N - S) / H) + 1 windows, window k reading the source ids [k H, k H + S) (the last one what is left); a window after
    the first is prompted with the r (S - H) stream ids from stream position r k H on, and every window but the last produces stream positions up to
    r k H + r S. Returns ``[(sequence, score_from, stream position of the first target)]``; ``stop_token``: appended to the last window's targets."""
    src, stream = list(src), list(stream)
    N = len(src)
    n = 1 if N <= S else -(-(N - S) // H) + 1
    rows = []
    for k in range(n):
        last = k == n - 1
        carry = r * (S - H) if k > 0 else 0
        first = r * k * H + carry
        targets = stream[first:] if last else stream[first:r * k * H + r * S]
        if last and stop_token is not None:
            targets = targets + [stop_token]
        if not targets:
            continue
        prompt = [i + semantic_offset for i in src[k * H:k * H + S]] + [infer_token] + stream[r * k * H:first]
        rows.append((np.asarray(prompt + targets, dtype=np.int32), len(prompt), first))
    return rows
