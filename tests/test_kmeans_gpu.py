"""GPU: the device k-means (csrc/kmeans.hip) against the float64 restatement in tests/kmeans_ref.py — E-step labels, the reproducible M-step with
relocation, greedy k-means++ picks and whole Lloyd fits."""
import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import kmeans as KM

from tests import kmeans_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _stream():
    return _cabi.current_stream_handle(DEV)


class Handle:
    def __init__(self, X: torch.Tensor, k: int, x_max_abs=None):
        self.lib = _cabi.load()
        n, d = X.shape
        self.h = self.lib.at_kmeans_create(0, n, d, k)
        assert self.h, _cabi.last_error()
        self.X = X
        mx = float(X.abs().max()) if x_max_abs is None else x_max_abs
        _cabi.check(self.lib.at_kmeans_set_data(self.h, X.data_ptr(), mx, _stream()), "set_data")

    def assign(self, C: torch.Tensor, c_max=-1.0):
        labels = torch.empty(self.X.shape[0], dtype=torch.int16, device=DEV)
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        _cabi.check(self.lib.at_kmeans_assign(self.h, C.data_ptr(), float(c_max), labels.data_ptr(), status.data_ptr(), _stream()), "assign")
        torch.cuda.synchronize()
        return labels.cpu().numpy().astype(np.int64), int(status.cpu()[0])

    def update(self, labels, C_old: torch.Tensor, prev=None):
        k = C_old.shape[0]
        lab = torch.from_numpy(np.asarray(labels, dtype=np.int16)).to(DEV)
        prv = None if prev is None else torch.from_numpy(np.asarray(prev, dtype=np.int16)).to(DEV)
        C_new = torch.empty_like(C_old)
        counts = torch.empty(k, dtype=torch.int32, device=DEV)
        stats = torch.zeros(6, dtype=torch.float64, device=DEV)
        _cabi.check(self.lib.at_kmeans_update(self.h, lab.data_ptr(), None if prv is None else prv.data_ptr(), C_old.data_ptr(), C_new.data_ptr(),
                                              counts.data_ptr(), stats.data_ptr(), _stream()), "update")
        reloc = torch.empty((k, 3), dtype=torch.int32, device=DEV)
        _cabi.check(self.lib.at_kmeans_relocations(self.h, reloc.data_ptr(), _stream()), "relocations")
        torch.cuda.synchronize()
        return C_new.cpu().numpy(), counts.cpu().numpy(), stats.cpu().numpy(), reloc.cpu().numpy()

    def close(self):
        self.lib.at_kmeans_destroy(self.h)


def _layernormed(n, d, seed):
    rng = np.random.default_rng(seed)
    h = rng.normal(0.0, 1.0, size=(n, d)) * rng.lognormal(0.0, 0.5, size=(1, d)) + rng.normal(0.0, 0.3, size=(1, d))
    h = (h - h.mean(axis=1, keepdims=True)) / np.sqrt(h.var(axis=1, keepdims=True) + 1e-5)
    return h.astype(np.float32)


def _centres_in_data(X, k, seed):
    """centres 'fitted to the data': data rows plus 1 % noise (near-ties on purpose)"""
    rng = np.random.default_rng(seed)
    rows = rng.choice(X.shape[0], size=k, replace=False)
    C = X[rows].astype(np.float64)
    C = C + 0.01 * np.abs(C).mean() * rng.normal(size=C.shape)
    return C.astype(np.float32)


def _refined_op(X, C):
    """at_op_gemm_split + at_op_vq_argmax_refined on the same rows and centres (the tokenizers' path, K padded to the GEMM's 128 columns)"""
    lib = _cabi.load()
    n, d = X.shape
    k = C.shape[0]
    kp = (k + 127) // 128 * 128
    Cp = torch.zeros((kp, d), dtype=torch.float32, device=DEV)
    Cp[:k] = C
    dots = torch.empty((n, kp), dtype=torch.float32, device=DEV)
    ws = torch.empty(((n + 255) // 256 * 256 + kp) * d * 2 * 2, dtype=torch.uint8, device=DEV)
    _cabi.check(lib.at_op_gemm_split(X.data_ptr(), Cp.data_ptr(), None, dots.data_ptr(), n, kp, d, 1, float(C.abs().max()), 0, ws.data_ptr(),
                                     ws.numel(), None, _stream()), "gemm_split")
    dk = dots[:, :k].contiguous()
    e2 = (C.double() ** 2).sum(dim=1).float().contiguous()
    out = torch.empty(n, dtype=torch.int16, device=DEV)
    _cabi.check(lib.at_op_vq_argmax_refined(X.data_ptr(), dk.data_ptr(), e2.data_ptr(), C.data_ptr(), out.data_ptr(), n, d, k, _stream()), "vq")
    torch.cuda.synchronize()
    return out.cpu().numpy().astype(np.int64)


@pytest.mark.parametrize("case", ["layernormed", "unnormalised"])
def test_assign_equals_float64_argmin(case):
    if case == "layernormed":
        n, d, k = 50_000, 1024, 2048
        X = _layernormed(n, d, 1)
    else:
        n, d, k = 20_000, 768, 1000
        X = (_layernormed(n, d, 2) * 300.0).astype(np.float32)   # |x| ~ 1e3
    C = _centres_in_data(X, k, 3)
    Xd = torch.from_numpy(X).to(DEV)
    Cd = torch.from_numpy(C).to(DEV)
    h = Handle(Xd, k)
    try:
        lab, status = h.assign(Cd, float(np.abs(C).max()))
    finally:
        h.close()
    assert status == 0
    ref = R.assign(X, C)
    bad = np.where(lab != ref)[0]
    assert bad.size == 0, f"{bad.size} rows differ from the float64 arg-min, first {bad[:5]} margins {[R.top2_margin(X[i], C) for i in bad[:5]]}"
    op = _refined_op(Xd, Cd)
    assert np.array_equal(lab, op)


def test_update_skewed_relocation_reproducible():
    n, d, k = 40_000, 256, 64
    rng = np.random.default_rng(5)
    X = rng.normal(0.0, 1.0, size=(n, d)).astype(np.float32)
    X[: n // 50] *= 8.0    # a few far rows: the relocation picks among them
    labels = rng.integers(0, k, size=n)
    labels[rng.random(n) < 0.4] = 0          # one cluster holds ~40 % of the rows
    labels[labels == 7] = 8                  # cluster 7 is empty
    labels[labels == 11] = 12                # and cluster 11
    C_old = rng.normal(0.0, 1.0, size=(k, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    Cd = torch.from_numpy(C_old).to(DEV)
    h = Handle(Xd, k)
    try:
        C1, cnt1, st1, rel1 = h.update(labels, Cd)
        C2, cnt2, st2, rel2 = h.update(labels, Cd)
    finally:
        h.close()
    ref = R.update(X, labels, C_old)
    assert np.array_equal(cnt1, ref["counts"])
    assert int(st1[3]) == ref["n_empty"] == 2
    got_rel = [tuple(int(v) for v in rel1[j]) for j in range(ref["n_empty"])]
    assert got_rel == ref["reloc"]
    ulp = np.spacing(np.abs(ref["centres"]).astype(np.float32))
    assert np.all(np.abs(C1.astype(np.float64) - ref["centres"].astype(np.float64)) <= ulp)
    assert abs(st1[0] - ref["inertia"]) <= 1e-12 * ref["inertia"]
    assert abs(st1[1] - ref["shift2"]) <= 1e-9 * ref["shift2"] + 1e-30
    assert np.array_equal(C1.view(np.uint32), C2.view(np.uint32))
    assert np.array_equal(st1.view(np.uint64), st2.view(np.uint64))
    assert np.array_equal(cnt1, cnt2)


def test_plusplus_picks_match_restatement():
    n, d, k = 20_000, 64, 256
    X, _ = R.mixture(n, d, 64, seed=7, spread=3.0)
    u = KM.plusplus_uniforms(k, 0)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        ud = torch.from_numpy(u).to(DEV)
        C = torch.empty((k, d), dtype=torch.float32, device=DEV)
        picked = torch.empty(k, dtype=torch.int64, device=DEV)
        _cabi.check(h.lib.at_kmeans_plusplus(h.h, ud.data_ptr(), u.shape[1], C.data_ptr(), picked.data_ptr(), _stream()), "plusplus")
        torch.cuda.synchronize()
        got = picked.cpu().numpy()
        Cg = C.cpu().numpy()
    finally:
        h.close()
    ref, margins = R.plusplus(X, u)
    assert np.array_equal(Cg, X[got])
    diff = np.where(got != ref)[0]
    if diff.size:
        s = int(diff[0])
        print(f"k-means++ first differs at centre {s}: device row {got[s]}, restatement row {ref[s]}, boundary margin {margins[s]:.3e} of the total")
        assert margins[s] < 1e-12, "a pick differs without a boundary tie"
    else:
        print(f"k-means++: all {k} picks equal; smallest boundary margin {margins[1:].min():.3e}")


def _fit(X, k, seed=0):
    km = KM.KMeans(k, init="k-means++", max_iter=150, tol=1e-4, seed=seed, device=DEV, record_labels=True)
    return km.fit(X)


def test_fit_matches_restatement_iteration_by_iteration():
    n, d, k = 100_000, 256, 512
    X, _ = R.mixture(n, d, k, seed=11, spread=1.0, noise=1.0)
    Xd = torch.from_numpy(X).to(DEV)
    km = _fit(Xd, k)
    km2 = _fit(Xd, k)
    assert np.array_equal(km.cluster_centers_.view(np.uint32), km2.cluster_centers_.view(np.uint32))
    assert np.array_equal(km.labels_, km2.labels_)
    assert km.n_iter_ == km2.n_iter_
    ref = R.lloyd(X, X[km.init_rows_], max_iter=150, tol=1e-4)
    for it, (a, b) in enumerate(zip(km.labels_history_, ref["labels_history"])):
        bad = np.where(a.astype(np.int64) != b)[0]
        if bad.size:
            i = int(bad[0])
            print(f"iteration {it}: {bad.size} labels differ; first row {i}: top-2 margin {R.top2_margin(X[i], ref['centres']):.3e}")
        assert bad.size == 0, f"labels differ at iteration {it}"
    assert km.n_iter_ == ref["n_iter"]
    h = np.array(km.inertia_history_)
    hr = np.array(ref["history"])
    assert np.all(np.abs(h - hr) <= 1e-12 * hr)
    assert np.allclose(km.cluster_centers_, ref["centres"], rtol=1e-6, atol=1e-6 * np.abs(ref["centres"]).max())
    assert np.array_equal(km.labels_.astype(np.int64), ref["labels"])
    assert np.array_equal(km.predict(Xd).astype(np.int64), km.labels_.astype(np.int64))
    assert np.all(km.counts_ > 0)
    print(f"fit: n_iter {km.n_iter_}, inertia {km.inertia_:.6e}")


@pytest.mark.parametrize("d", [768, 1024])
def test_update_and_plusplus_at_the_tokenizer_widths(d):
    n, k = 12_000, 64
    X, _ = R.mixture(n, d, 48, seed=d, spread=2.0)
    rng = np.random.default_rng(d)
    labels = rng.integers(0, k, size=n)
    labels[labels == 3] = 4                  # one empty cluster
    C_old = rng.normal(0.0, 1.0, size=(k, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        C1, cnt1, st1, rel1 = h.update(labels, torch.from_numpy(C_old).to(DEV))
        u = KM.plusplus_uniforms(k, 1)
        ud = torch.from_numpy(u).to(DEV)
        C = torch.empty((k, d), dtype=torch.float32, device=DEV)
        picked = torch.empty(k, dtype=torch.int64, device=DEV)
        _cabi.check(h.lib.at_kmeans_plusplus(h.h, ud.data_ptr(), u.shape[1], C.data_ptr(), picked.data_ptr(), _stream()), "plusplus")
        torch.cuda.synchronize()
        got = picked.cpu().numpy()
    finally:
        h.close()
    ref = R.update(X, labels, C_old)
    assert np.array_equal(cnt1, ref["counts"])
    assert [tuple(int(v) for v in rel1[j]) for j in range(ref["n_empty"])] == ref["reloc"]
    ulp = np.spacing(np.abs(ref["centres"]).astype(np.float32))
    assert np.all(np.abs(C1.astype(np.float64) - ref["centres"].astype(np.float64)) <= ulp)
    assert abs(st1[0] - ref["inertia"]) <= 1e-12 * ref["inertia"]
    pr, margins = R.plusplus(X, u)
    diff = np.where(got != pr)[0]
    if diff.size:
        print(f"k-means++ (D {d}) first differs at centre {diff[0]}: boundary margin {margins[diff[0]]:.3e}")
        assert margins[diff[0]] < 1e-12


def test_assign_on_the_bf16x3_scheme():
    n, d, k = 10_000, 768, 1000
    X = _layernormed(n, d, 9)
    C = _centres_in_data(X, k, 10)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        _cabi.check(h.lib.at_kmeans_set_option(h.h, b"scheme", 0), "set_option")
        assert h.lib.at_kmeans_get_option(h.h, b"scheme") == 0
        _cabi.check(h.lib.at_kmeans_set_data(h.h, Xd.data_ptr(), float(np.abs(X).max()), _stream()), "set_data")
        lab, status = h.assign(torch.from_numpy(C).to(DEV))
    finally:
        h.close()
    assert status == 0
    assert np.array_equal(lab, R.assign(X, C))


def test_assign_on_tiny_magnitudes():
    n, d, k = 8_000, 256, 256
    X = (_layernormed(n, d, 12) * 1e-5).astype(np.float32)
    C = _centres_in_data(X, k, 13)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        lab, status = h.assign(torch.from_numpy(C).to(DEV), float(np.abs(C).max()))
    finally:
        h.close()
    assert status == 0
    assert np.array_equal(lab, R.assign(X, C))


def test_predict_fewer_rows_than_clusters():
    X, _ = R.mixture(4_000, 64, 32, seed=21, spread=4.0)
    km = KM.KMeans(128, seed=2, max_iter=20, device=DEV).fit(X)
    few = X[:50]
    pred = km.predict(few).astype(np.int64)
    assert np.array_equal(pred, km.labels_[:50].astype(np.int64))
    assert np.array_equal(pred, R.assign(few, km.cluster_centers_))
