"""Device k-means for fitting the semantic tokenizers' code books (csrc/kmeans.hip through the C ABI).

``KMeans`` follows ``sklearn.cluster.KMeans(algorithm="lloyd")``: greedy k-means++ (or random rows, or given centres), Lloyd iterations until the labels
stop changing, the centre shift falls to ``tol * mean(var(X, axis=0))`` or ``max_iter`` is reached, empty clusters relocated by sklearn's rule, and a final
E-step so that ``predict(X_fit) == labels_``. Every device step is a HIP kernel; the host reads six numbers per iteration. The uniforms of k-means++ come
from the counter-based stream of ``prng.py`` (``("kmeans++", seed + i)``), so ``tests/kmeans_ref.py`` restates a fit in numpy.

``save_vq`` / ``save_kmeans`` write the files the tokenizers' loaders read (``load_w2vbert_checkpoint`` / ``load_hubert_checkpoint``).
"""
from __future__ import annotations

import math
import os
from typing import Optional

import numpy as np

from . import prng

MAX_K = 32767
STATUS_F16_OVERFLOW, STATUS_NONFINITE = 2, 4


def check_shape(n: int, d: int, k: int) -> None:
    """The constraints of the device k-means (include/audiotoken_hip.h, at_kmeans_*)."""
    if d < 64 or d % 64 or d > 1024:
        raise ValueError(f"k-means: D = {d}; D must be a multiple of 64 in [64, 1024]")
    if k < 4 or k > MAX_K or k % 4:
        raise ValueError(f"k-means: K = {k}; K must be a multiple of 4 in [4, {MAX_K}]")
    if n < k:
        raise ValueError(f"k-means: N = {n} rows < K = {k} clusters")


def n_local_trials(k: int) -> int:
    return 2 + int(np.log(k))


def plusplus_uniforms(k: int, seed: int) -> np.ndarray:
    """[K][trials] float64 uniforms in [0, 1) (53 bits) of stream ("kmeans++", seed): row 0 column 0 picks the first centre."""
    t = n_local_trials(k)
    return prng.uniform01_f64("kmeans++", k * t, seed).reshape(k, t)


def random_rows(n: int, k: int, seed: int) -> np.ndarray:
    """K distinct rows by a seeded host permutation ("random" init)."""
    return np.random.default_rng(seed).permutation(n)[:k]


def column_variance_mean(Xd, rows: int = 65536) -> float:
    """mean(var(X, axis=0)) in float64, over row chunks (sklearn's _tolerance)."""
    import torch
    n, d = Xd.shape
    s = torch.zeros(d, dtype=torch.float64, device=Xd.device)
    for r in range(0, n, rows):
        s += Xd[r:r + rows].double().sum(dim=0)
    mean = s / n
    q = torch.zeros(d, dtype=torch.float64, device=Xd.device)
    for r in range(0, n, rows):
        q += ((Xd[r:r + rows].double() - mean) ** 2).sum(dim=0)
    return float((q / n).mean().item())


def tolerance(x_var_mean: float, tol: float) -> float:
    return float(x_var_mean) * float(tol)


class KMeans:
    """Full-batch Lloyd k-means on one HIP device. ``X``: float32 [N, D] (a device tensor or a host array)."""

    def __init__(self, n_clusters: int, *, init="k-means++", n_init: int = 1, max_iter: int = 150, tol: float = 1e-4, seed: int = 0,
                 device: str = "cuda:0", record_labels: bool = False):
        if not (isinstance(init, np.ndarray) or init in ("k-means++", "random")):
            raise ValueError(f"init must be 'k-means++', 'random' or an array, not {init!r}")
        if int(n_init) < 1 or int(max_iter) < 1:
            raise ValueError("n_init and max_iter must be >= 1")
        self.n_clusters = int(n_clusters)
        self.init = init
        self.n_init = int(n_init)
        self.max_iter = int(max_iter)
        self.tol = float(tol)
        self.seed = int(seed)
        self.device = device
        self.record_labels = bool(record_labels)   # keep every iteration's labels (host int16) in labels_history_: for tests
        self.cluster_centers_: Optional[np.ndarray] = None
        self.labels_: Optional[np.ndarray] = None
        self.counts_: Optional[np.ndarray] = None
        self.inertia_: Optional[float] = None
        self.inertia_history_: list = []
        self.labels_history_: list = []
        self.n_iter_: Optional[int] = None
        self.init_rows_: Optional[np.ndarray] = None
        self.fit_summary_: dict = {}
        self.scheme_fallbacks_ = 0

    # pickles without device state: everything above is host data
    def __getstate__(self):
        return dict(self.__dict__)

    def __setstate__(self, state):
        self.__dict__.update(state)

    # ---- device plumbing -----------------------------------------------------------------------------------------------------------------------
    def _device_rows(self, X):
        import torch
        dev = torch.device(self.device)
        if isinstance(X, torch.Tensor):
            t = X.detach()
            if t.device != dev:
                t = t.to(dev)
        else:
            t = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float32))).to(dev)
        if t.dtype != torch.float32 or t.dim() != 2:
            raise ValueError(f"X must be float32 [N, D], got {tuple(t.shape)} {t.dtype}")
        return t.contiguous()

    def _open(self, Xd):
        import torch
        from . import _cabi
        lib = _cabi.load()
        n, d = Xd.shape
        check_shape(n, d, self.n_clusters)
        dev = torch.device(self.device)
        h = lib.at_kmeans_create(dev.index or 0, n, d, self.n_clusters)
        if not h:
            raise _cabi.HipLibraryError(f"at_kmeans_create failed: {_cabi.last_error()}")
        return lib, h

    # ---- the fit ---------------------------------------------------------------------------------------------------------------------------------
    def fit(self, X, x_max_abs: Optional[float] = None):
        from . import _cabi
        shape = tuple(np.shape(X)) if not hasattr(X, "shape") else tuple(X.shape)
        if len(shape) != 2:
            raise ValueError(f"X must be [N, D], got shape {shape}")
        check_shape(shape[0], shape[1], self.n_clusters)   # before anything touches a device
        Xd = self._device_rows(X)
        n, d = Xd.shape
        k = self.n_clusters
        if isinstance(self.init, np.ndarray) and self.init.shape != (k, d):
            raise ValueError(f"init array must be [{k}, {d}], got {self.init.shape}")
        if x_max_abs is None:
            x_max_abs = float(Xd.abs().max().item())
        if not math.isfinite(x_max_abs):
            raise ValueError("X holds a NaN or an infinity")
        x_var_mean = column_variance_mean(Xd)
        tol_abs = tolerance(x_var_mean, self.tol)
        lib, h = self._open(Xd)
        try:
            stream = _cabi.current_stream_handle(self.device)
            _cabi.check(lib.at_kmeans_set_data(h, Xd.data_ptr(), float(x_max_abs), stream), "at_kmeans_set_data")
            best = None
            for run in range(self.n_init):
                res = self._single(lib, h, Xd, x_max_abs, tol_abs, self.seed + run, stream)
                if best is None or res["inertia"] < best["inertia"]:
                    best = res
        finally:
            lib.at_kmeans_destroy(h)
        self.cluster_centers_ = best["centres"]
        self.labels_ = best["labels"]
        self.counts_ = np.bincount(self.labels_.astype(np.int64), minlength=k).astype(np.int64)
        self.inertia_ = best["inertia"]
        self.inertia_history_ = best["history"]
        self.labels_history_ = best["labels_history"]
        self.n_iter_ = best["n_iter"]
        self.init_rows_ = best["init_rows"]
        return self

    def _single(self, lib, h, Xd, x_max_abs, tol_abs, seed, stream):
        import torch
        from . import _cabi
        n, d = Xd.shape
        k = self.n_clusters
        dev = Xd.device
        init_rows = None
        c_max = -1.0   # first E-step: max |X| bounds centres drawn from the rows
        if isinstance(self.init, np.ndarray):
            C = torch.from_numpy(np.ascontiguousarray(self.init, dtype=np.float32)).to(dev)
            c_max = float(np.abs(self.init).max())   # given centres need not lie inside the data's range
        elif self.init == "random":
            init_rows = random_rows(n, k, seed)
            C = Xd[torch.from_numpy(init_rows).to(dev)].contiguous()
        else:
            u = torch.from_numpy(plusplus_uniforms(k, seed)).to(dev)
            C = torch.empty((k, d), dtype=torch.float32, device=dev)
            picked = torch.empty(k, dtype=torch.int64, device=dev)
            _cabi.check(lib.at_kmeans_plusplus(h, u.data_ptr(), u.shape[1], C.data_ptr(), picked.data_ptr(), stream), "at_kmeans_plusplus")
            init_rows = picked.cpu().numpy()
        C_new = torch.empty_like(C)
        labels = torch.empty(n, dtype=torch.int16, device=dev)
        prev = torch.empty(n, dtype=torch.int16, device=dev)
        counts = torch.empty(k, dtype=torch.int32, device=dev)
        stats = torch.zeros(6, dtype=torch.float64, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        stats_h = torch.empty(6, dtype=torch.float64).pin_memory()
        status_h = torch.empty(1, dtype=torch.int32).pin_memory()
        history, labels_hist = [], []
        have_prev = False
        n_iter = 0
        for it in range(self.max_iter):
            while True:
                _cabi.check(lib.at_kmeans_assign(h, C.data_ptr(), float(c_max), labels.data_ptr(), status.data_ptr(), stream), "at_kmeans_assign")
                _cabi.check(lib.at_kmeans_update(h, labels.data_ptr(), prev.data_ptr() if have_prev else None, C.data_ptr(), C_new.data_ptr(),
                                                 counts.data_ptr(), stats.data_ptr(), stream), "at_kmeans_update")
                stats_h.copy_(stats, non_blocking=True)
                status_h.copy_(status, non_blocking=True)
                torch.cuda.current_stream(dev).synchronize()   # the one host sync of an iteration
                if not self._fallback(lib, h, int(status_h[0]), Xd, x_max_abs, stream):
                    break
            inertia, shift2, n_changed, n_empty, c_max, n_invalid = (float(v) for v in stats_h.tolist())
            if n_invalid:
                raise RuntimeError(f"k-means: {int(n_invalid)} labels outside [0, {k})")
            history.append(inertia)
            if self.record_labels:
                labels_hist.append(labels.cpu().numpy())
            n_iter = it + 1
            C, C_new = C_new, C
            if have_prev and n_changed == 0:    # strict convergence
                break
            if shift2 <= tol_abs:
                break
            labels, prev = prev, labels
            have_prev = True
        # final E-step against the final centres: predict(X_fit) == labels_ by construction; the inertia of those labels
        self._assign(lib, h, C, c_max, labels, status, status_h, stream, Xd, x_max_abs)
        _cabi.check(lib.at_kmeans_update(h, labels.data_ptr(), None, C.data_ptr(), C_new.data_ptr(), counts.data_ptr(), stats.data_ptr(), stream),
                    "at_kmeans_update")
        final_inertia = float(stats.cpu()[0])
        return {"centres": C.cpu().numpy().copy(), "labels": labels.cpu().numpy().copy(), "inertia": final_inertia, "history": history,
                "labels_history": labels_hist, "n_iter": n_iter, "init_rows": init_rows}

    def _fallback(self, lib, h, st, Xd, x_max_abs, stream) -> bool:
        """Act on an E-step's status word: True = the step must be repeated (now on three bf16 pieces)."""
        from . import _cabi
        if st & STATUS_NONFINITE:
            raise ValueError("k-means: a row or a centre holds a NaN or an infinity")
        if st & STATUS_F16_OVERFLOW:
            if lib.at_kmeans_get_option(h, b"scheme") == 0:
                raise RuntimeError("k-means: range overflow on the bf16x3 scheme")
            # the two-piece fp16 operands do not hold these values: repeat on three bf16 pieces (any magnitude) and stay there
            _cabi.check(lib.at_kmeans_set_option(h, b"scheme", 0), "at_kmeans_set_option")
            _cabi.check(lib.at_kmeans_set_data(h, Xd.data_ptr(), float(x_max_abs), stream), "at_kmeans_set_data")
            self.scheme_fallbacks_ += 1
            return True
        return False

    def _assign(self, lib, h, C, c_max, labels, status, status_h, stream, Xd, x_max_abs):
        import torch
        from . import _cabi
        while True:
            _cabi.check(lib.at_kmeans_assign(h, C.data_ptr(), float(c_max), labels.data_ptr(), status.data_ptr(), stream), "at_kmeans_assign")
            status_h.copy_(status, non_blocking=True)
            torch.cuda.current_stream(Xd.device).synchronize()
            if not self._fallback(lib, h, int(status_h[0]), Xd, x_max_abs, stream):
                return

    def predict(self, X, x_max_abs: Optional[float] = None) -> np.ndarray:
        """Nearest fitted centre of every row (the fit's own E-step)."""
        import torch
        from . import _cabi
        if self.cluster_centers_ is None:
            raise RuntimeError("KMeans.predict before fit")
        Xd = self._device_rows(X)
        n = Xd.shape[0]
        if n < self.n_clusters:   # a handle needs N >= K rows: zero rows pad the call, their labels are dropped
            Xd = torch.cat([Xd, torch.zeros((self.n_clusters - n, Xd.shape[1]), dtype=Xd.dtype, device=Xd.device)])
        if x_max_abs is None:
            x_max_abs = float(Xd.abs().max().item())
        lib, h = self._open(Xd)
        try:
            stream = _cabi.current_stream_handle(self.device)
            _cabi.check(lib.at_kmeans_set_data(h, Xd.data_ptr(), float(x_max_abs), stream), "at_kmeans_set_data")
            C = torch.from_numpy(np.ascontiguousarray(self.cluster_centers_, dtype=np.float32)).to(Xd.device)
            labels = torch.empty(Xd.shape[0], dtype=torch.int16, device=Xd.device)
            status = torch.zeros(1, dtype=torch.int32, device=Xd.device)
            status_h = torch.empty(1, dtype=torch.int32).pin_memory()
            c_max = float(np.abs(self.cluster_centers_).max())
            self._assign(lib, h, C, c_max, labels, status, status_h, stream, Xd, x_max_abs)
            return labels[:n].cpu().numpy()
        finally:
            lib.at_kmeans_destroy(h)


# ---- writers in the tokenizers' formats ----------------------------------------------------------------------------------------------------------
def save_vq(path: os.PathLike, centres: np.ndarray) -> None:
    """semantic_m: the VectorQuantize state-dict key ``load_w2vbert_checkpoint`` reads, ``{"_codebook.embed": float32 [1, K, D]}``."""
    import torch
    c = np.ascontiguousarray(np.asarray(centres, dtype=np.float32))
    if c.ndim != 2:
        raise ValueError(f"centres must be [K, D], got {c.shape}")
    torch.save({"_codebook.embed": torch.from_numpy(c.copy()).unsqueeze(0)}, os.fspath(path))


def save_kmeans(path: os.PathLike, km: KMeans) -> None:
    """semantic_s: ``joblib.dump`` of the fitted estimator, whose ``cluster_centers_`` ``load_hubert_checkpoint`` reads."""
    import joblib
    if km.cluster_centers_ is None:
        raise ValueError("save_kmeans: the estimator is not fitted")
    joblib.dump(km, os.fspath(path))
