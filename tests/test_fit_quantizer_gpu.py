"""GPU: AudioToken.fit_quantizer end to end. Synthetic checkpoints written as directories (as tests/test_checkpoint_files_gpu.py writes them), 16
speech-like 10 s clips as WAV files; the code book fitted without a quantizer, then the tokenizer loaded WITH the fitted file must reproduce the fit's own
final assignment on every frame; a different batch size / worker count must give bit-identical centres."""
import json
import os

import numpy as np
import pytest
import torch

from audiotoken_amd import weights as W
from audiotoken_amd.synthetic import speech_like_waveform

pytestmark = pytest.mark.gpu

NL = 3   # conformer / transformer layers of the fixtures


def _write_dir(d, sd, arch, model_type, prefix=""):
    from safetensors.torch import save_file
    os.makedirs(d, exist_ok=True)
    save_file({prefix + k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in sd.items()}, os.path.join(d, "model.safetensors"))
    with open(os.path.join(d, "config.json"), "w") as fh:
        json.dump(dict(arch, model_type=model_type, num_hidden_layers=NL), fh)


def _clips(tmp_path, sr=16000):
    from scipy.io import wavfile
    d = tmp_path / "corpus"
    d.mkdir()
    x = speech_like_waveform(16, 10 * sr, sr, seed=77)
    for i in range(16):
        wavfile.write(str(d / f"clip{i:02d}.wav"), sr, x[i].astype(np.float32))
    return d


def _checkpoint(tmp_path, which):
    if which == "semantic_m":
        from audiotoken_amd.encoder import W2VBERT_ARCH
        w = W.synth_w2vbert_weights(n_layers=NL, seed=5, with_vq=False)
        d = str(tmp_path / "w2vbert2_l21")
        _write_dir(d, {k: v for k, v in w.items() if not k.startswith("vq.")}, W2VBERT_ARCH, "wav2vec2-bert")
        return d, "vq.pkl", 2048
    from audiotoken_amd.hubert import HUBERT_ARCH
    w = W.synth_hubert_weights(NL, 6, False)
    d = str(tmp_path / "mhubert-base")
    _write_dir(d, {k: v for k, v in w.items() if not k.startswith("kmeans.")}, HUBERT_ARCH, "hubert", prefix="hubert.")
    return d, "km.bin", 1000


def _tok(which, **kw):
    from audiotoken_amd import AudioToken, Tokenizers
    t = AudioToken(Tokenizers(which), device="cuda:0", **kw)
    t.model_config.output_layer = NL
    return t


@pytest.mark.parametrize("which", ["semantic_m", "semantic_s"])
def test_fitted_quantizer_reproduces_the_fit_assignment(cuda_device, tmp_path, which):
    corpus = _clips(tmp_path)
    ckpt, qname, k = _checkpoint(tmp_path, which)
    qpath = str(tmp_path / qname)
    km = _tok(which, weights=ckpt).fit_quantizer(qpath, audio_dir=str(corpus), chunk_size=30, batch_size=4, num_workers=0, max_iter=30, seed=0)
    assert km.cluster_centers_.shape[0] == k and os.path.exists(qpath)
    assert km.fit_summary_["frames"] == len(km.labels_) and not km.fit_summary_["truncated"]
    out = tmp_path / "tokens"
    _tok(which, weights=ckpt, quantizer=qpath).encode_batch_files(batch_size=4, outdir=str(out), audio_dir=str(corpus), chunk_size=30, num_workers=0)
    saved = np.concatenate([np.load(out / f"clip{i:02d}.npy").reshape(-1) for i in range(16)]).astype(np.int64)
    assert saved.shape == km.labels_.shape
    bad = np.where(saved != km.labels_.astype(np.int64))[0]
    assert bad.size == 0, f"{bad.size} of {saved.size} frames differ, first {bad[:8]}"
    used = np.unique(km.labels_).size
    print(f"{which}: {saved.size} frames, {used} of {k} codes used, n_iter {km.n_iter_}")
    assert used == k


def test_fit_is_independent_of_batching(cuda_device, tmp_path):
    corpus = _clips(tmp_path)
    ckpt, qname, _ = _checkpoint(tmp_path, "semantic_m")
    a = _tok("semantic_m", weights=ckpt).fit_quantizer(str(tmp_path / "a.pkl"), audio_dir=str(corpus), batch_size=4, num_workers=0, max_iter=10,
                                                       keep_fraction=0.7, seed=3)
    b = _tok("semantic_m", weights=ckpt).fit_quantizer(str(tmp_path / "b.pkl"), audio_dir=str(corpus), batch_size=6, num_workers=2, max_iter=10,
                                                       keep_fraction=0.7, seed=3)
    assert a.fit_summary_["frames"] == b.fit_summary_["frames"] < a.fit_summary_["frames_seen"]
    assert np.array_equal(a.cluster_centers_.view(np.uint32), b.cluster_centers_.view(np.uint32))
    assert np.array_equal(a.labels_, b.labels_)
