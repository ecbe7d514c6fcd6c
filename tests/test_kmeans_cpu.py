"""CPU: the float64 k-means restatement (tests/kmeans_ref.py) against sklearn, the code-book writers read back through the loaders' own code, the
argument checks of the device k-means and the pickling of a KMeans without a device."""
import pickle

import numpy as np
import pytest

from audiotoken_amd import kmeans as KM

from tests import kmeans_ref as R


def test_restatement_matches_sklearn_lloyd():
    sk = pytest.importorskip("sklearn.cluster")
    X, _ = R.mixture(3000, 16, 12, seed=3, spread=8.0, dtype=np.float64)
    C0 = X[np.random.default_rng(0).choice(len(X), 12, replace=False)]
    ref = R.lloyd(X, C0, max_iter=300, tol=1e-4, fp32_centres=False)
    km = sk.KMeans(n_clusters=12, init=C0, n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X)
    assert np.array_equal(km.labels_, ref["labels"])
    assert np.allclose(km.cluster_centers_, ref["centres"], rtol=0, atol=1e-12 * np.abs(X).max())
    assert km.n_iter_ == ref["n_iter"]
    assert abs(km.inertia_ - ref["inertia"]) <= 1e-10 * ref["inertia"]


class _GivenUniforms:
    """A stand-in for sklearn's RandomState that hands _kmeans_plusplus the device's uniforms: the first centre floor(u[0, 0] N), then row c of u"""

    def __init__(self, u):
        self.u, self.c = u, 0

    def choice(self, n, p=None):
        return min(int(np.floor(self.u[0, 0] * n)), n - 1)

    def uniform(self, size=None):
        self.c += 1
        assert size == self.u.shape[1]
        return self.u[self.c].copy()


def test_restatement_degenerate_data_matches_sklearn():
    """Fewer distinct rows than K (integer rows: every distance is exact in float64, so sklearn's expanded form sees the same ties): k-means++ reaches
    zero potential and picks row 0 from then on, the E-step gives exact ties to the lower index, and the fit ends with sklearn's partition of the rows,
    number of distinct clusters and (up to sklearn's own rounding) inertia 0."""
    sk = pytest.importorskip("sklearn.cluster")
    from sklearn.cluster import _kmeans
    rng = np.random.default_rng(7)
    P = rng.integers(-3, 4, size=(9, 8)).astype(np.float64)
    P[:, 0] = 8.0 * np.arange(9)
    X = P[rng.integers(0, 9, size=400)]
    k = 24
    u = KM.plusplus_uniforms(k, 3)
    picked, margins = R.plusplus(X, u)
    _, sk_picked = _kmeans._kmeans_plusplus(X, k, np.einsum("ij,ij->i", X, X), np.ones(len(X)), _GivenUniforms(u), n_local_trials=u.shape[1])
    assert np.array_equal(picked, sk_picked)
    assert len(np.unique(X[picked], axis=0)) == 9 and np.all(picked[9:] == 0) and np.isinf(margins[9:]).all()
    # all rows equal: zero potential from the second centre on
    Z = np.zeros((50, 8))
    z_picked, z_margins = R.plusplus(Z, u)
    _, sk_z = _kmeans._kmeans_plusplus(Z, k, np.zeros(50), np.ones(50), _GivenUniforms(u), n_local_trials=u.shape[1])
    assert np.array_equal(z_picked, sk_z) and np.all(z_picked[1:] == 0) and np.isinf(z_margins[1:]).all()
    # E-step over duplicate centres: sklearn's labels (strict <, the lower index); then the whole fit. sklearn warns about finding fewer distinct
    # clusters than K.
    import warnings
    C = X[picked].astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        est = sk.KMeans(n_clusters=k, init=C.astype(np.float64), n_init=1, max_iter=1).fit(X)   # fitted attributes for predict(); centres replaced
        est.cluster_centers_ = C.astype(np.float64)
        assert np.array_equal(est.predict(X), R.assign(X, C))
        km = sk.KMeans(n_clusters=k, init=C.astype(np.float64), n_init=1, algorithm="lloyd", max_iter=300, tol=1e-4).fit(X)
    ref = R.lloyd(X, C, max_iter=300, tol=1e-4, fp32_centres=False)
    assert ref["inertia"] == 0.0 and km.inertia_ <= 1e-20   # (sklearn's expanded-form inertia leaves ~1e-26)
    assert len(np.unique(ref["labels"])) == len(np.unique(km.labels_)) == 9

    def partition(lab):
        return sorted(tuple(np.where(lab == j)[0]) for j in np.unique(lab))
    assert partition(ref["labels"]) == partition(km.labels_) == partition(np.unique(X, axis=0, return_inverse=True)[1].ravel())


def test_restatement_relocates_empty_clusters_like_the_rule():
    rng = np.random.default_rng(1)
    X = rng.normal(size=(200, 8))
    labels = rng.integers(0, 4, size=200)
    labels[labels == 2] = 1
    C = rng.normal(size=(6, 8)).astype(np.float32)   # clusters 2, 4, 5 empty
    m = R.update(X, labels, C)
    d2 = ((X - C.astype(np.float64)[labels]) ** 2).sum(axis=1)
    far = np.argsort(-d2, kind="stable")[:3]
    assert [r for r, _, _ in m["reloc"]] == list(far)
    assert [nw for _, _, nw in m["reloc"]] == [2, 4, 5]
    assert np.all(m["counts"] > 0) and m["counts"].sum() == 200
    for r, _, nw in m["reloc"]:
        assert np.array_equal(m["centres"][nw], X[r].astype(np.float32))


def test_writers_read_back_through_the_loaders(tmp_path):
    import joblib
    import torch
    rng = np.random.default_rng(2)
    C = rng.normal(size=(2048, 1024)).astype(np.float32)
    KM.save_vq(tmp_path / "vq.pkl", C)
    sd = torch.load(tmp_path / "vq.pkl", map_location="cpu", weights_only=True)
    assert tuple(sd["_codebook.embed"].shape) == (1, 2048, 1024)
    assert np.array_equal(sd["_codebook.embed"][0].numpy(), C)
    km = KM.KMeans(1000, device="cuda:0")
    km.cluster_centers_ = rng.normal(size=(1000, 768)).astype(np.float32)
    KM.save_kmeans(tmp_path / "km.pkl", km)
    back = joblib.load(tmp_path / "km.pkl")
    assert np.array_equal(np.asarray(back.cluster_centers_, dtype=np.float32), km.cluster_centers_)
    with pytest.raises(ValueError):
        KM.save_kmeans(tmp_path / "none.pkl", KM.KMeans(8))


@pytest.mark.parametrize("n,d,k", [(100, 100, 8), (100, 1088, 8), (100, 32, 8), (100, 64, 6), (100, 64, 2), (40000, 64, 32768), (7, 64, 8)])
def test_shape_validation(n, d, k):
    with pytest.raises(ValueError):
        KM.check_shape(n, d, k)
    with pytest.raises(ValueError):
        KM.KMeans(k).fit(np.zeros((n, d), dtype=np.float32))


def test_shape_validation_accepts_the_tokenizer_sizes():
    KM.check_shape(4096, 1024, 2048)
    KM.check_shape(4096, 768, 1000)


def test_device_bytes_and_c_abi_validation():
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    assert lib.at_kmeans_device_bytes(1 << 20, 1024, 2048) > (1 << 20) * 1024 * 4   # the fp16 pieces of X alone are 4 D bytes a row
    assert lib.at_kmeans_device_bytes(1000, 100, 8) == 0
    assert lib.at_kmeans_device_bytes(1000, 64, 1002) == 0
    assert not lib.at_kmeans_create(0, 100, 64, 200)
    assert "N" in _cabi.last_error() or "K" in _cabi.last_error()


def test_uniforms_are_the_counter_stream():
    u = KM.plusplus_uniforms(2048, 5)
    assert u.shape == (2048, KM.n_local_trials(2048)) == (2048, 9)
    from audiotoken_amd import prng
    assert np.array_equal(u.ravel(), prng.uniform01_f64("kmeans++", u.size, 5))
    assert np.all((u >= 0) & (u < 1))


def test_init_validation():
    with pytest.raises(ValueError):
        KM.KMeans(8, init="kmeans||")
    with pytest.raises(ValueError):
        KM.KMeans(8, n_init=0)


def test_pickles_before_and_after_a_fit_without_a_device():
    km = KM.KMeans(16, init="random", seed=3, device="cuda:7")
    back = pickle.loads(pickle.dumps(km))
    assert back.n_clusters == 16 and back.init == "random" and back.cluster_centers_ is None
    # a fitted estimator is host data only
    km.cluster_centers_ = np.ones((16, 64), np.float32)
    km.labels_ = np.zeros(100, np.int16)
    km.counts_ = np.full(16, 6)
    km.inertia_, km.n_iter_, km.inertia_history_ = 1.0, 3, [3.0, 2.0, 1.0]
    back = pickle.loads(pickle.dumps(km))
    assert np.array_equal(back.cluster_centers_, km.cluster_centers_) and back.n_iter_ == 3 and back.inertia_history_ == [3.0, 2.0, 1.0]


def test_kmeans_is_exported_lazily():
    import audiotoken_amd
    assert audiotoken_amd.KMeans is KM.KMeans


def test_fit_quantizer_argument_validation(tmp_path):
    from audiotoken_amd import AudioToken, Tokenizers
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.acoustic, device="cuda:0").fit_quantizer(tmp_path / "q.pkl", audio_dir=str(tmp_path))
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.semantic_m, device="cuda:0").fit_quantizer(tmp_path / "q.pkl", audio_dir=str(tmp_path), num_clusters=1024)
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.semantic_s, device="cuda:0").fit_quantizer(tmp_path / "q.pkl", audio_dir=str(tmp_path), num_clusters=2048)
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.semantic_s, device="cuda:0").fit_quantizer(tmp_path / "q.pkl", audio_dir=str(tmp_path), keep_fraction=0.0)
    with pytest.raises(ValueError):
        AudioToken(Tokenizers.semantic_m, device="cuda:0").fit_quantizer(tmp_path / "q.pkl", audio_dir=str(tmp_path), max_frames=100)


def test_uniforms_resolve_more_than_2_24_rows():
    u = KM.plusplus_uniforms(4096, 0)
    assert np.any(np.abs(u * 2.0 ** 24 - np.round(u * 2.0 ** 24)) > 0)   # not float32 values
