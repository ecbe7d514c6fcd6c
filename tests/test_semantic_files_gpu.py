"""GPU: ``AudioToken.to_audio_batch_files`` (audiotoken_amd/semantic_files.py) on a small tree of semantic token files, with a 2-layer
synthetic GPT at ``window=8, hop=4, max_new_tokens=12`` (as tests/test_gpt_queue_gpu.py) and fine model "a" of tests/fine_cases.py. The route is checked
stage by stage against the calls it is made of: the round's ``to_acoustic`` with the files' stacked draws, ``to_fine`` on each file alone with its own
draws, and ``decode_batch_files`` of the acoustic tokenizer on the codes the run saved."""
import os
import shutil

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd import semantic_files as SF
from audiotoken_amd import weights as W
from audiotoken_amd.configs import Wav2VecBertDecoderConfig
from audiotoken_amd.fine_decoder import fine_windows

from tests import fine_cases

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GEN = dict(window=8, hop=4, max_new_tokens=12, slots=8, fine_slots=4, seed=5)
VALID = ["a/s0", "a/s1", "a/s2", "a/s3", "b/sub/s0", "b/sub/s1", "b/sub/s2", "b/sub/s3", "b/sub/s4", "b/t0"]    # sorted as the run walks them
BAD = {"a/float": "dtype", "a/past": "outside", "b/empty": "empty"}
_cache = {}


def source(i):
    """9 to 17 ids: 2 to 4 windows at (8, 4), so every source has at least the 12 frames of its first window."""
    return ((np.arange(9 + (5 * i) % 9) * 7 + i) % 1000).astype(np.int64)


def make_tree(root, names=VALID, bad=True):
    for i, name in enumerate(VALID):
        if name in names:
            os.makedirs(os.path.dirname(os.path.join(root, name)), exist_ok=True)
            a = source(i)
            np.save(os.path.join(root, name + ".npy"), (a.astype(np.int16), a[None], a[None, None])[i % 3])    # every accepted rank and dtype
    if bad:
        np.save(os.path.join(root, "a/float.npy"), source(1).astype(np.float32))
        np.save(os.path.join(root, "a/past.npy"), np.array([1, 2, Wav2VecBertDecoderConfig().SEMANTIC_VOCAB_SIZE, 4], dtype=np.int64))
        np.save(os.path.join(root, "b/empty.npy"), np.zeros((1, 0), dtype=np.int64))


def tokenizer():
    if "sem" not in _cache:
        gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
        _cache["sem"] = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))
        _cache["ac"] = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8)
    return _cache["sem"], _cache["ac"]


def read_all(root, ext):
    out = {}
    for d, _, names in os.walk(root):
        for n in names:
            if n.endswith(ext):
                p = os.path.join(d, n)
                with open(p, "rb") as f:
                    out[os.path.relpath(p, root)[:-len(ext)].replace(os.sep, "/")] = f.read()
    return out


@pytest.fixture(scope="module")
def main_run(tmp_path_factory):
    """The run every test below looks at: the whole tree, ``round_files=4``, WAV, one clip per file."""
    sem, _ = tokenizer()
    base = tmp_path_factory.mktemp("semantic_files")
    tree, out, codes = str(base / "tree"), str(base / "out"), str(base / "codes")
    make_tree(tree)
    sem.to_audio_batch_files(3, out, token_dir=tree, round_files=4, codes_dir=codes, **GEN)
    return dict(base=base, tree=tree, out=out, codes=codes, summary=dict(sem.run_summary), timings=dict(sem.run_timings), skipped=list(sem.skipped_files))


def test_outputs_skips_and_summary(main_run):
    wavs = read_all(main_run["out"], ".wav")
    assert sorted(wavs) == sorted(VALID), "one output per valid file at the mirrored path, none for the others"
    skipped = {os.path.relpath(p, main_run["tree"])[:-4].replace(os.sep, "/"): why for p, why in main_run["skipped"]}
    assert sorted(skipped) == sorted(BAD)
    for name, text in BAD.items():
        assert text in skipped[name], (name, skipped[name])
    codes = {k: np.load(os.path.join(main_run["codes"], k + ".npy")) for k in VALID}
    s = main_run["summary"]
    assert s["files"] == 10 and s["skipped_files"] == 3 and s["rounds"] == 3 and s["gpt_ticks"] > 0 and s["fine_passes"] >= 3
    assert s["generated_frames"] == sum(c.shape[1] for c in codes.values())
    for k, c in codes.items():
        assert c.dtype == np.int16 and c.shape[0] == 8 and len(wavs[k]) == 44 + 2 * 320 * c.shape[1]
    assert main_run["timings"]["gpt_s"] > 0 and main_run["timings"]["fine_s"] > 0
    # a second input that maps to the same output name is skipped: two directories written flat
    sem, _ = tokenizer()
    flat = str(main_run["base"] / "flat")
    files = [os.path.join(main_run["tree"], n + ".npy") for n in ("a/s0", "b/sub/s0", "a/s1")]
    sem.to_audio_batch_files(2, flat, token_files=files, **GEN)
    assert sorted(read_all(flat, ".wav")) == ["s0", "s1"] and len(sem.skipped_files) == 1
    assert sem.skipped_files[0][0] == files[1] and "duplicate output name" in sem.skipped_files[0][1]


def test_each_stage_is_the_call_it_is_made_of(main_run):
    sem, _ = tokenizer()
    stages = SF.Stages(sem, GEN["seed"], 0.8, 100, 0.5, GEN["max_new_tokens"], GEN["window"], GEN["hop"], GEN["slots"], GEN["fine_slots"])
    for r in range(0, len(VALID), 4):
        names = VALID[r:r + 4]
        srcs = [source(VALID.index(n)) for n in names]
        caps = [stages.capacity(len(s)) for s in srcs]
        u = SF.stack_gpt_draws([SF.file_draws(GEN["seed"], n, cap)[0] for n, cap in zip(names, caps)])
        coarse = sem.to_acoustic(srcs, long_form=True, slots=8, window=8, hop=4, max_new_tokens=12, uniforms=u)
        for n, cap, c in zip(names, caps, coarse.codes):
            saved = torch.from_numpy(np.load(os.path.join(main_run["codes"], n + ".npy")).astype(np.int64))
            assert torch.equal(saved[:2], c), f"{n}: the coarse codes are those of the round's to_acoustic call with the files' draws"
            fu = SF.file_draws(GEN["seed"], n, cap, len(fine_windows(c.shape[1], 128)), 128)[1]
            alone = sem.to_fine(c, uniforms=fu[None])
            assert torch.equal(saved, alone.codes[0]), f"{n}: the saved codes are to_fine on its coarse codes alone with its file draws"


@pytest.mark.parametrize("mode", ["wav", "flac", "stream", "rescale_chunked"])
def test_audio_is_decode_batch_files_on_the_saved_codes(main_run, mode):
    sem, ac = tokenizer()
    base = main_run["base"]
    kw = {"wav": dict(), "flac": dict(audio_format="flac"), "stream": dict(stream=True, chunk_size=0.1), "rescale_chunked": dict(rescale=True, chunk_size=0.1)}[mode]
    ext = ".flac" if mode == "flac" else ".wav"
    if mode == "wav":
        got_dir, codes = main_run["out"], main_run["codes"]
    else:
        got_dir, codes = str(base / f"out_{mode}"), str(base / f"codes_{mode}")
        sem.to_audio_batch_files(3, got_dir, token_dir=main_run["tree"], round_files=4, codes_dir=codes, **GEN, **kw)
        assert read_all(codes, ".npy") == read_all(main_run["codes"], ".npy"), "the codes do not depend on how they are decoded"
    want_dir = str(base / f"want_{mode}")
    ac.decode_batch_files(3, want_dir, token_dir=codes, **{"chunk_size": None, **kw})
    got, want = read_all(got_dir, ext), read_all(want_dir, ext)
    assert sorted(got) == sorted(VALID) == sorted(want)
    for k in VALID:
        assert got[k] == want[k], f"{k}: other bytes than decode_batch_files writes from the saved codes"
    assert ac.run_summary["files"] == 10


def test_round_size_and_renaming(main_run):
    """Round 0's four files alone in a tree, at another ``round_files``: the same members, so the same bytes. Then one of them renamed: another key, so
    other draws and another file; the others still follow the rule with their own, unchanged draws."""
    sem, _ = tokenizer()
    base = main_run["base"]
    first = read_all(main_run["out"], ".wav")
    tree, out = str(base / "tree0"), str(base / "out0")
    make_tree(tree, VALID[:4], bad=False)
    sem.to_audio_batch_files(3, out, token_dir=tree, round_files=9, **GEN)
    again = read_all(out, ".wav")
    assert sorted(again) == VALID[:4] and all(again[k] == first[k] for k in VALID[:4])
    assert sem.run_summary["rounds"] == 1
    os.rename(os.path.join(tree, "a/s1.npy"), os.path.join(tree, "a/s1x.npy"))     # keeps its place in the walk
    out, codes = str(base / "out1"), str(base / "codes1")
    sem.to_audio_batch_files(3, out, token_dir=tree, round_files=9, codes_dir=codes, **GEN)
    renamed = read_all(out, ".wav")
    assert sorted(renamed) == ["a/s0", "a/s1x", "a/s2", "a/s3"] and renamed["a/s1x"] != first["a/s1"]
    assert not np.array_equal(SF.file_draws(5, "a/s1x", 40)[0], SF.file_draws(5, "a/s1", 40)[0])
    stages = SF.Stages(sem, GEN["seed"], 0.8, 100, 0.5, GEN["max_new_tokens"], GEN["window"], GEN["hop"], GEN["slots"], GEN["fine_slots"])
    for n in ("a/s0", "a/s2", "a/s3"):
        saved = torch.from_numpy(np.load(os.path.join(codes, n + ".npy")).astype(np.int64))
        cap = stages.capacity(len(source(VALID.index(n))))
        fu = SF.file_draws(GEN["seed"], n, cap, len(fine_windows(saved.shape[1], 128)), 128)[1]
        assert torch.equal(saved, sem.to_fine(saved[:2], uniforms=fu[None]).codes[0])
    shutil.rmtree(tree)
