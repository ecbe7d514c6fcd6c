"""Float64 numpy restatement of the device k-means (audiotoken_amd/kmeans.py, csrc/kmeans.hip): greedy k-means++ with the same uniforms, Lloyd's E- and
M-steps, sklearn's relocation of empty clusters (farthest rows first, ties to the lower row; empty clusters in increasing index order) and its tolerance
rule. ``fp32_centres=True`` rounds every new centre to float32 once, as the device does.

Degenerate data (duplicate rows, fewer distinct rows than K, all rows equal) follows sklearn where sklearn defines the outcome: k-means++ at zero potential
searches u * 0 = 0 and so picks row 0, as sklearn's searchsorted does; trials of equal potential (duplicate rows) keep the first trial, as
sklearn's argmin; E-step ties go to the lower centre index (sklearn's strict <). Where sklearn leaves
the order open (its relocation takes np.argpartition of the distances), the device's documented rule holds: equal distances relocate the lower row first.
Rows are read in blocks and widened to float64 per block, so float32 data of millions of rows needs no float64 copy."""
from __future__ import annotations

from concurrent.futures import ThreadPoolExecutor

import numpy as np

_THREADS = 8   # row blocks of the distance passes in parallel (numpy releases the GIL inside them)


def sq_dist_rows(X: np.ndarray, c: np.ndarray, block: int = 65536) -> np.ndarray:
    c = np.asarray(c, dtype=np.float64)
    out = np.empty(X.shape[0], dtype=np.float64)

    def rows(r):
        d = np.asarray(X[r:r + block], dtype=np.float64) - c[None, :]
        out[r:r + block] = np.einsum("ij,ij->i", d, d)
    if X.shape[0] <= block:
        rows(0)
    else:
        with ThreadPoolExecutor(_THREADS) as pool:
            list(pool.map(rows, range(0, X.shape[0], block)))
    return out


def plusplus(X: np.ndarray, uniforms: np.ndarray):
    """Greedy k-means++ (sklearn _kmeans_plusplus) in float64. Returns (picked rows, per-step smallest |scan - u total| / total over the trials).
    At zero potential every search is for 0, found at row 0 whatever the rounding: its margin is infinite."""
    X = np.asarray(X)
    n = X.shape[0]
    k, trials = uniforms.shape
    first = min(int(np.floor(uniforms[0, 0] * n)), n - 1)
    picked = [first]
    closest = sq_dist_rows(X, X[first])
    margins = [np.inf]
    for c in range(1, k):
        cs = np.cumsum(closest)
        total = cs[-1]
        vals = uniforms[c] * total
        ids = np.minimum(np.searchsorted(cs, vals, side="left"), n - 1)
        # how close each search was to a boundary of the scan: a device scan that differs in the last bits can only pick another row below this
        lo = np.where(ids > 0, cs[np.maximum(ids - 1, 0)], 0.0)
        margins.append(float(np.min(np.minimum(np.abs(cs[ids] - vals), np.abs(vals - lo)) / total)) if total > 0 else np.inf)
        best_pot, best_id, best_d = None, None, None
        for cid in ids:
            d = np.minimum(closest, sq_dist_rows(X, X[cid]))
            pot = d.sum()
            if best_pot is None or pot < best_pot:   # ties to the first trial (sklearn's argmin): duplicate rows tie
                best_pot, best_id, best_d = pot, int(cid), d
        picked.append(best_id)
        closest = best_d
    return np.array(picked, dtype=np.int64), np.array(margins)


def assign(X: np.ndarray, C: np.ndarray, block: int = 8192) -> np.ndarray:
    """Exact float64 arg-min of |x - c|^2, ties to the lower index (the expanded form, rows near a tie re-evaluated from differences)."""
    X = np.asarray(X, dtype=np.float64)
    C = np.asarray(C, dtype=np.float64)
    c2 = np.einsum("ij,ij->i", C, C)
    out = np.empty(X.shape[0], dtype=np.int64)
    for r in range(0, X.shape[0], block):
        xb = X[r:r + block]
        d = (np.einsum("ij,ij->i", xb, xb)[:, None] + c2[None, :]) - 2.0 * (xb @ C.T)
        lab = np.argmin(d, axis=1)
        best = d[np.arange(len(xb)), lab]
        near = d <= best[:, None] + 1e-9 * np.maximum(np.abs(best)[:, None], 1.0)
        for i in np.where(near.sum(axis=1) > 1)[0]:
            cand = np.where(near[i])[0]
            ex = ((xb[i][None, :] - C[cand]) ** 2).sum(axis=1)
            lab[i] = cand[int(np.argmin(ex))]   # first minimum: the lower index on an exact tie
        out[r:r + block] = lab
    return out


def top2_margin(x: np.ndarray, C: np.ndarray) -> float:
    """(second smallest - smallest) / smallest exact squared distance of one row."""
    d = np.sort(((np.asarray(C, np.float64) - np.asarray(x, np.float64)[None, :]) ** 2).sum(axis=1))
    return float((d[1] - d[0]) / max(d[0], 1e-300))


def update(X: np.ndarray, labels: np.ndarray, C_old: np.ndarray, fp32_centres: bool = True):
    """One M-step. Returns dict(centres, counts, inertia, shift2, n_empty, reloc [(row, old, new)], rowd2)."""
    X = np.asarray(X, dtype=np.float64)
    n, d = X.shape
    k = C_old.shape[0]
    labels = np.asarray(labels, dtype=np.int64)
    counts = np.bincount(labels, minlength=k).astype(np.int64)
    order = np.argsort(labels, kind="stable")
    sums = np.zeros((k, d), dtype=np.float64)
    starts = np.concatenate([[0], np.cumsum(counts)[:-1]])
    for j in np.where(counts > 0)[0]:
        sums[j] = X[order[starts[j]:starts[j] + counts[j]]].sum(axis=0)
    Co = np.asarray(C_old, dtype=np.float64)
    diff = X - Co[labels]
    rowd2 = np.einsum("ij,ij->i", diff, diff)
    inertia = float(rowd2.sum())
    empty = np.where(counts == 0)[0]
    reloc = []
    if len(empty):
        far = np.lexsort((np.arange(n), -rowd2))[:len(empty)]   # distance descending, row ascending
        for new, r in zip(empty, far):
            old = int(labels[r])
            sums[old] -= X[r]
            counts[old] -= 1
            sums[new] = X[r]
            counts[new] = 1
            reloc.append((int(r), old, int(new)))
    cnt = counts.astype(np.float64)[:, None]
    C_new = np.where(cnt > 0, sums / np.maximum(cnt, 1.0), sums)
    if fp32_centres:
        C_new = C_new.astype(np.float32)
    shift2 = float(((np.asarray(C_new, np.float64) - Co) ** 2).sum())
    return {"centres": C_new, "counts": counts, "inertia": inertia, "shift2": shift2, "n_empty": int(len(empty)), "reloc": reloc, "rowd2": rowd2}


def tolerance(X: np.ndarray, tol: float) -> float:
    return float(np.mean(np.var(np.asarray(X, dtype=np.float64), axis=0))) * tol


def lloyd(X: np.ndarray, C0: np.ndarray, max_iter: int = 150, tol: float = 1e-4, fp32_centres: bool = True):
    """sklearn's Lloyd loop (strict convergence, centre-shift tolerance, max_iter) and a final E-step. Returns dict(centres, labels, inertia, n_iter,
    history [inertia per iteration], labels_history)."""
    C = np.asarray(C0, dtype=np.float32 if fp32_centres else np.float64).copy()
    tol_abs = tolerance(X, tol)
    prev = None
    history, labels_hist = [], []
    n_iter = 0
    for it in range(max_iter):
        labels = assign(X, C)
        m = update(X, labels, C, fp32_centres)
        history.append(m["inertia"])
        labels_hist.append(labels)
        n_iter = it + 1
        C = m["centres"]
        if prev is not None and np.array_equal(prev, labels):
            break
        if m["shift2"] <= tol_abs:
            break
        prev = labels
    labels = assign(X, C)
    diff = np.asarray(X, np.float64) - np.asarray(C, np.float64)[labels]
    return {"centres": C, "labels": labels, "inertia": float(np.einsum("ij,ij->", diff, diff)), "n_iter": n_iter, "history": history,
            "labels_history": labels_hist}


def mixture(n: int, d: int, k: int, seed: int = 0, spread: float = 10.0, noise: float = 1.0, dtype=np.float32):
    """A Gaussian mixture of k components (seeded numpy generator): rows, true component of each row."""
    rng = np.random.default_rng(seed)
    means = rng.normal(0.0, spread, size=(k, d))
    comp = rng.integers(0, k, size=n)
    X = means[comp] + rng.normal(0.0, noise, size=(n, d))
    return X.astype(dtype), comp
