"""GPU: the device k-means (csrc/kmeans.hip) against the float64 restatement (tests/kmeans_ref.py) where its dispatch and its data change path —
every width bucket of the per-lane row registers (KM_BY_Q: Q = ceil(D / 256), partial and full widths), K from 4 to 32764 (the scatter's large-LDS
branch, a one-row last E-step chunk), N past 2^22 rows (the k-means++ search walks several segments per thread), degenerate data (duplicate rows,
fewer distinct rows than K, all rows equal or zero) and the host paths of KMeans (the fp16-range fall-back, random / given / repeated inits, the
changed-label and invalid-label counts). The bars are those of tests/test_kmeans_gpu.py; every case prints its worst error or differing count."""
import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd import kmeans as KM

from tests import kmeans_ref as R
from tests.test_kmeans_gpu import DEV, Handle, _centres_in_data, _layernormed, _stream

pytestmark = pytest.mark.gpu


def _q(d):
    return (d + 255) // 256


def _width(d):
    return f"D {d} (Q={_q(d)}, {'full' if d % 256 == 0 else 'partial'} width)"


def _plusplus(h, k, seed):
    u = KM.plusplus_uniforms(k, seed)
    ud = torch.from_numpy(u).to(DEV)
    d = h.X.shape[1]
    C = torch.empty((k, d), dtype=torch.float32, device=DEV)
    picked = torch.empty(k, dtype=torch.int64, device=DEV)
    _cabi.check(h.lib.at_kmeans_plusplus(h.h, ud.data_ptr(), u.shape[1], C.data_ptr(), picked.data_ptr(), _stream()), "plusplus")
    torch.cuda.synchronize()
    return u, picked.cpu().numpy(), C.cpu().numpy()


def _check_assign(tag, X, C, lab, status, block=8192):
    assert status == 0, f"{tag}: status {status}"
    ref = R.assign(X, C, block=block)
    bad = np.where(lab != ref)[0]
    print(f"{tag}: assign N {len(X)} K {len(C)}: {bad.size} labels differ from the float64 arg-min")
    assert bad.size == 0, f"{tag}: first rows {bad[:5]} margins {[R.top2_margin(X[i], C) for i in bad[:5]]}"


def _check_update(tag, X, labels, C_old, got, ref):
    C1, cnt, st, rel = got
    assert np.array_equal(cnt, ref["counts"]), f"{tag}: {int((cnt != ref['counts']).sum())} counts differ"
    assert int(st[3]) == ref["n_empty"]
    got_rel = [tuple(int(v) for v in rel[j]) for j in range(ref["n_empty"])]
    assert got_rel == ref["reloc"], f"{tag}: relocations differ"
    ulp = np.spacing(np.abs(ref["centres"]).astype(np.float32))
    cerr = np.abs(C1.astype(np.float64) - ref["centres"].astype(np.float64))
    ierr = abs(st[0] - ref["inertia"]) / max(ref["inertia"], 1e-300)
    print(f"{tag}: update: n_empty {ref['n_empty']}, largest cluster {int(ref['counts'].max())} rows, worst centre error {float((cerr / ulp).max()):.2f} ulp, "
          f"inertia rel err {ierr:.1e}")
    assert np.all(cerr <= ulp), f"{tag}: {int((cerr > ulp).sum())} centre entries beyond one ulp"
    assert ierr <= 1e-12 or (ref["inertia"] == 0.0 and st[0] == 0.0)


def _check_plusplus(tag, X, u, got, Cg):
    assert np.array_equal(Cg, X[got])
    ref, margins = R.plusplus(X, u)
    diff = np.where(got != ref)[0]
    if diff.size:
        s = int(diff[0])
        print(f"{tag}: k-means++ first differs at centre {s} of {len(got)}: boundary margin {margins[s]:.3e}")
        assert margins[s] < 1e-12, f"{tag}: a pick differs without a boundary tie"
    else:
        print(f"{tag}: k-means++: all {len(got)} picks equal; smallest boundary margin {margins[1:].min() if len(got) > 1 else np.inf:.3e}")


# ---- every width bucket ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [64, 128, 192, 256, 320, 448, 512, 576, 640, 768, 832, 960, 1024])
def test_assign_update_plusplus_at_every_width(d):
    n, k = 6000, 64
    X = _layernormed(n, d, 100 + d)
    C = _centres_in_data(X, k, 200 + d)
    rng = np.random.default_rng(d)
    labels = rng.integers(0, k, size=n)
    labels[rng.random(n) < 0.12] = 0          # cluster 0: ~800 rows, two 512-row parts
    labels[labels == 5] = 6                   # cluster 5 empty
    C_old = rng.normal(0.0, 1.0, size=(k, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        lab, status = h.assign(torch.from_numpy(C).to(DEV), float(np.abs(C).max()))
        got1 = h.update(labels, torch.from_numpy(C_old).to(DEV))
        got2 = h.update(labels, torch.from_numpy(C_old).to(DEV))
        u, picked, Cg = _plusplus(h, k, d)
    finally:
        h.close()
    tag = _width(d)
    _check_assign(tag, X, C, lab, status)
    ref = R.update(X, labels, C_old)
    assert ref["counts"][0] > 512 and ref["n_empty"] == 1
    _check_update(tag, X, labels, C_old, got1, ref)
    for a, b in zip(got1, got2):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), f"{tag}: repeated update differs"
    _check_plusplus(tag, X, u, picked, Cg)


def _fit_vs_restatement(tag, X, km, C0):
    """the device fit iteration by iteration against R.lloyd from the same initial centres"""
    ref = R.lloyd(X, C0, max_iter=km.max_iter, tol=km.tol)
    for it, (a, b) in enumerate(zip(km.labels_history_, ref["labels_history"])):
        bad = np.where(a.astype(np.int64) != b)[0]
        if bad.size:
            print(f"{tag}: iteration {it}: {bad.size} labels differ; first row {int(bad[0])}")
        assert bad.size == 0, f"{tag}: labels differ at iteration {it}"
    assert km.n_iter_ == ref["n_iter"], f"{tag}: n_iter {km.n_iter_} != {ref['n_iter']}"
    h, hr = np.array(km.inertia_history_), np.array(ref["history"])
    assert np.all(np.abs(h - hr) <= 1e-12 * hr)
    assert np.array_equal(km.labels_.astype(np.int64), ref["labels"])
    ulp = np.spacing(np.abs(ref["centres"]).astype(np.float32))
    cerr = np.abs(km.cluster_centers_.astype(np.float64) - ref["centres"].astype(np.float64))
    print(f"{tag}: fit: n_iter {km.n_iter_}, inertia {km.inertia_:.6e} (restatement {ref['inertia']:.6e}), worst centre error "
          f"{float((cerr / ulp).max()):.2f} ulp")
    assert np.all(cerr <= ulp)
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-12 * ref["inertia"] or km.inertia_ == ref["inertia"] == 0.0
    return ref


@pytest.mark.parametrize("d", [448, 832])
def test_fit_iteration_by_iteration_at_partial_widths(d):
    n, k = 30_000, 128
    X, _ = R.mixture(n, d, k, seed=d, spread=1.0, noise=1.0)
    km = KM.KMeans(k, seed=3, device=DEV, record_labels=True).fit(X)
    _fit_vs_restatement(_width(d), X, km, X[km.init_rows_])


# ---- K and N limits --------------------------------------------------------------------------------------------------------------------------------
def test_largest_k_scatter_lds_and_one_row_chunk():
    n, d, k = 9 * 4096 + 1, 64, 32764
    rng = np.random.default_rng(32764)
    X = rng.normal(0.0, 1.0, size=(n, d)).astype(np.float32)
    C = (X[rng.choice(n, size=k, replace=False)] + 0.05 * rng.normal(size=(k, d))).astype(np.float32)
    labels = np.arange(n) % k                 # one or two rows per cluster
    gone = rng.choice(k, size=40, replace=False)
    labels[np.isin(labels, gone)] = (labels[np.isin(labels, gone)] + 1) % k
    gone = np.setdiff1d(gone, np.unique(labels))   # a neighbour of an emptied cluster may have been refilled
    C_old = rng.normal(0.0, 1.0, size=(k, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        chunk = h.lib.at_kmeans_get_option(h.h, b"chunk_rows")
        lab, status = h.assign(torch.from_numpy(C).to(DEV), float(np.abs(C).max()))
        got = h.update(labels, torch.from_numpy(C_old).to(DEV))
    finally:
        h.close()
    assert chunk == 4096 and n % chunk == 1, "the last E-step chunk is one row"
    tag = f"K {k} N {n} D {d} (scatter LDS {k * 4} B)"
    _check_assign(tag, X, C, lab, status, block=256)
    ref = R.update(X, labels, C_old)
    assert ref["n_empty"] == len(gone) >= 35
    _check_update(tag, X, labels, C_old, got, ref)


@pytest.mark.parametrize("n,d,k", [(300, 64, 4), (4000, 320, 12), (12, 128, 12), (200, 576, 200), (9000, 192, 2052)])
def test_small_odd_and_padded_k(n, d, k):
    """K = 4 and 12 (fewer code rows than one vq_argmax wave reads), K = 2052 (Kpad = 2176), N == K, N < 256"""
    X, _ = R.mixture(n, d, max(2, min(k, n // 4)), seed=n + k, spread=2.0)
    rng = np.random.default_rng(k)
    C = _centres_in_data(X, k, k)
    labels = rng.integers(0, k, size=n)
    labels[labels == k - 1] = 0               # the last cluster empty
    C_old = rng.normal(0.0, 1.0, size=(k, d)).astype(np.float32)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        lab, status = h.assign(torch.from_numpy(C).to(DEV), float(np.abs(C).max()))
        got = h.update(labels, torch.from_numpy(C_old).to(DEV))
        pp = _plusplus(h, k, 7) if k <= 256 else None   # (K = 2052 seeds 2051 centres: tens of seconds of float64 restatement for no new path)
    finally:
        h.close()
    tag = f"N {n} D {d} K {k}"
    _check_assign(tag, X, C, lab, status)
    ref = R.update(X, labels, C_old)
    assert ref["n_empty"] >= 1
    _check_update(tag, X, labels, C_old, got, ref)
    if pp is not None:
        u, picked, Cg = pp
        _check_plusplus(tag, X, u, picked, Cg)
        if n == k:
            assert np.array_equal(np.sort(picked), np.arange(n)), "N == K distinct rows: k-means++ picks every row once"


def test_plusplus_past_2_22_rows():
    n, d, k = (1 << 22) + 4113, 64, 8
    assert (n + 4095) // 4096 > 1024, "more segments than the search kernel's threads"
    rng = np.random.default_rng(22)
    X = rng.standard_normal(size=(n, d), dtype=np.float32)
    X[rng.integers(0, n, size=64)] *= 6.0    # a few far rows: large, uneven segment totals
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        u, picked, Cg = _plusplus(h, k, 22)
    finally:
        h.close()
    _check_plusplus(f"N {n} (nseg {(n + 4095) // 4096}) D {d} K {k}", X, u, picked, Cg)


# ---- degenerate data -------------------------------------------------------------------------------------------------------------------------------
def _distinct_points(m, d, seed):
    """m well separated integer points: exact float arithmetic, no near-ties between distinct points"""
    rng = np.random.default_rng(seed)
    P = rng.integers(-3, 4, size=(m, d)).astype(np.float32)
    P[:, 0] = 8.0 * np.arange(m)
    return P


def test_duplicate_rows_and_duplicate_centres():
    n, d, k = 5000, 128, 32
    P = _distinct_points(50, d, 1)
    rng = np.random.default_rng(2)
    X = P[rng.integers(0, 50, size=n)]
    C = P[rng.choice(50, size=k, replace=False)].copy()
    C[[9, 20, 31]] = C[4]                     # exact duplicate centres: ties to the lower index
    C[[12, 25]] = C[0]
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        lab, status = h.assign(torch.from_numpy(C).to(DEV), float(np.abs(C).max()))
        u, picked, Cg = _plusplus(h, k, 5)
    finally:
        h.close()
    _check_assign("duplicate rows, duplicate centres", X, C, lab, status)
    assert not np.isin(lab, [9, 20, 31, 12, 25]).any()
    assert np.any(lab == 4) and np.any(lab == 0)
    _check_plusplus("duplicate rows", X, u, picked, Cg)
    km = KM.KMeans(k, seed=4, device=DEV, record_labels=True).fit(X)
    _fit_vs_restatement("duplicate rows", X, km, X[km.init_rows_])


def test_fewer_distinct_rows_than_clusters_fit():
    n, d, k = 3000, 64, 128
    P = _distinct_points(20, d, 3)
    X = P[np.random.default_rng(4).integers(0, 20, size=n)]
    km = KM.KMeans(k, seed=1, device=DEV, record_labels=True).fit(X)
    u = KM.plusplus_uniforms(k, 1)
    ref_rows, margins = R.plusplus(X, u)
    assert np.array_equal(km.init_rows_, ref_rows), "k-means++ past zero potential picks row 0 (sklearn's searchsorted of 0)"
    assert np.isinf(margins[20:]).all()
    ref = _fit_vs_restatement("20 distinct rows, K 128", X, km, X[km.init_rows_])
    assert km.inertia_ == 0.0 and len(np.unique(km.labels_)) == 20
    assert len(ref["history"]) == km.n_iter_


@pytest.mark.parametrize("value", [0.0, 1.5])
def test_all_rows_equal(value):
    n, d, k = 2000, 192, 16
    X = np.full((n, d), value, dtype=np.float32)
    if value:
        X[:, ::3] = -value
    km = KM.KMeans(k, seed=2, device=DEV, record_labels=True).fit(X)
    u = KM.plusplus_uniforms(k, 2)
    ref_rows, _ = R.plusplus(X, u)
    assert np.array_equal(km.init_rows_, ref_rows)
    _fit_vs_restatement(f"all rows {'zero' if value == 0 else 'equal'}", X, km, X[km.init_rows_])
    assert km.inertia_ == 0.0 and np.all(km.labels_ == 0)


def test_relocating_a_cluster_s_only_member():
    n, d, k = 3000, 320, 16
    rng = np.random.default_rng(6)
    X = rng.normal(0.0, 1.0, size=(n, d)).astype(np.float32)
    C_old = rng.normal(0.0, 0.1, size=(k, d)).astype(np.float32)
    labels = rng.integers(0, 8, size=n)       # clusters 8 .. 15 empty
    far = 1234
    X[far] *= 10.0                            # the farthest row of all ...
    labels[far] = 3
    labels[(labels == 3) & (np.arange(n) != far)] = 4   # ... is cluster 3's only member
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        got = h.update(labels, torch.from_numpy(C_old).to(DEV))
    finally:
        h.close()
    ref = R.update(X, labels, C_old)
    assert ref["reloc"][0] == (far, 3, 8) and ref["counts"][3] == 0
    _check_update("only member relocated", X, labels, C_old, got, ref)
    assert got[1][3] == 0 and np.all(got[0][3] == 0.0)


# ---- host paths of KMeans --------------------------------------------------------------------------------------------------------------------------
def test_fp16_range_fallback():
    n, d, k = 8000, 256, 32
    X, _ = R.mixture(n, d, k, seed=31, spread=2000.0, noise=300.0)   # |x| ~ 1e4: beyond fp16 under any scale of max |x| = 1
    km = KM.KMeans(k, seed=5, device=DEV, record_labels=True).fit(X, x_max_abs=1.0)
    print(f"understated x_max_abs: scheme_fallbacks_ {km.scheme_fallbacks_} (max |x| {np.abs(X).max():.3e})")
    assert km.scheme_fallbacks_ == 1
    _fit_vs_restatement("bf16x3 after the fall-back", X, km, X[km.init_rows_])


def test_random_and_array_init():
    n, d, k = 10_000, 128, 64
    X, _ = R.mixture(n, d, k, seed=41, spread=1.5)
    km = KM.KMeans(k, init="random", seed=9, device=DEV, record_labels=True).fit(X)
    assert np.array_equal(km.init_rows_, KM.random_rows(n, k, 9))
    _fit_vs_restatement("init random", X, km, X[km.init_rows_])
    C0 = (np.random.default_rng(10).normal(0.0, 40.0, size=(k, d))).astype(np.float32)   # far outside the data (|x| <~ 10)
    assert np.abs(C0).max() > 4 * np.abs(X).max()
    km = KM.KMeans(k, init=C0, seed=0, device=DEV, record_labels=True).fit(X)
    _fit_vs_restatement("init array", X, km, C0)


def test_n_init_keeps_the_best_of_the_restated_runs():
    n, d, k = 8000, 64, 48
    X, _ = R.mixture(n, d, 40, seed=51, spread=1.0)
    km = KM.KMeans(k, n_init=3, seed=20, device=DEV).fit(X)
    runs = []
    for s in range(20, 23):
        rows, _ = R.plusplus(X, KM.plusplus_uniforms(k, s))
        runs.append((R.lloyd(X, X[rows]), rows))
    inertias = [r["inertia"] for r, _ in runs]
    best = int(np.argmin(inertias))
    print(f"n_init 3: restated inertias {[f'{v:.6e}' for v in inertias]}, device {km.inertia_:.6e}")
    assert np.array_equal(km.init_rows_, runs[best][1])
    assert abs(km.inertia_ - inertias[best]) <= 1e-12 * inertias[best]
    assert np.array_equal(km.labels_.astype(np.int64), runs[best][0]["labels"])


def test_update_changed_and_invalid_label_counts():
    n, d, k = 20_000, 576, 40
    rng = np.random.default_rng(61)
    X = rng.normal(0.0, 1.0, size=(n, d)).astype(np.float32)
    labels = np.arange(n) % k
    rng.shuffle(labels)
    prev = labels.copy()
    moved = rng.random(n) < 0.07
    prev[moved] = (prev[moved] + 1 + rng.integers(0, k - 1, size=int(moved.sum()))) % k
    C_old = rng.normal(0.0, 0.5, size=(k, d)).astype(np.float32)
    bad = labels.copy()
    inv = rng.choice(n, size=150, replace=False)
    bad[inv[:70]] = -1
    bad[inv[70:]] = k
    valid = (bad >= 0) & (bad < k)
    Xd = torch.from_numpy(X).to(DEV)
    h = Handle(Xd, k)
    try:
        got_prev = h.update(labels, torch.from_numpy(C_old).to(DEV), prev=prev)
        got_bad = h.update(bad, torch.from_numpy(C_old).to(DEV))
    finally:
        h.close()
    n_changed = int((labels != prev).sum())
    print(f"prev_labels: stats[2] {got_prev[2][2]:.0f}, numpy {n_changed}; invalid labels: stats[5] {got_bad[2][5]:.0f}, numpy {int((~valid).sum())}")
    assert got_prev[2][2] == n_changed and got_prev[2][5] == 0
    _check_update("with prev_labels", X, labels, C_old, got_prev, R.update(X, labels, C_old))
    assert got_bad[2][5] == int((~valid).sum()) == 150
    ref = R.update(X[valid], bad[valid], C_old)
    assert ref["n_empty"] == 0
    _check_update("labels -1 and K", X[valid], bad[valid], C_old, got_bad, ref)
