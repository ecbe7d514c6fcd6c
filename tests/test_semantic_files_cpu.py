"""CPU: what ``AudioToken.to_audio_batch_files`` (audiotoken_amd/semantic_files.py) does without a device: the per-file draw rule, the
reading and skipping of semantic token files, the round planning of ``SemanticRun`` against a stub generator and a stub decoder (host writer), and the
interface's refusals."""
import os

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd import semantic_files as SF
from audiotoken_amd.runs import RunLog
from audiotoken_amd.writer import TokenFileError, output_path


def test_file_draws_rule():
    assert SF.fnv1a64("") == 0xCBF29CE484222325 and SF.fnv1a64("a") == 0xAF63DC4C8601EC8C and SF.fnv1a64("foobar") == 0x85944171F73967E8
    gpt, fine = SF.file_draws(7, "a/b/clip", 50, 3, 128)
    assert gpt.dtype == np.float32 and gpt.shape == (50,) and fine.dtype == np.float32 and fine.shape == (3, 6, 128)
    g = np.random.Generator(np.random.Philox(key=[7, SF.fnv1a64("a/b/clip")]))
    assert np.array_equal(gpt, g.random(50, dtype=np.float32)) and np.array_equal(fine, g.random((3, 6, 128), dtype=np.float32)), "the documented rule"
    again = SF.file_draws(7, "a/b/clip", 50, 3, 128)
    assert np.array_equal(again[0], gpt) and np.array_equal(again[1], fine), "deterministic"
    assert np.array_equal(SF.file_draws(7, "a/b/clip", 50)[0], gpt) and SF.file_draws(7, "a/b/clip", 50)[1].shape == (0, 6, 0)
    assert np.array_equal(SF.file_draws(7, "a/b/clip", 50, 5, 128)[1][:3], fine), "a longer result keeps the draws of its first windows"
    for seed, stem in ((8, "a/b/clip"), (7, "a/b/clip2"), (7, "a/clip")):
        other = SF.file_draws(seed, stem, 50, 3, 128)
        assert not np.array_equal(other[0], gpt) and not np.array_equal(other[1], fine), "another seed or another stem: other draws"
    # a file's draws do not depend on the other keys: drawing for other files in between changes nothing
    for stem in ("x", "y", "a/b/clip3"):
        SF.file_draws(7, stem, 99, 2, 256)
    assert np.array_equal(SF.file_draws(7, "a/b/clip", 50, 3, 128)[1], fine)
    u = SF.stack_gpt_draws([gpt[:3], gpt])
    assert u.shape == (2, 50) and np.array_equal(u[0, :3], gpt[:3]) and not u[0, 3:].any() and np.array_equal(u[1], gpt)
    assert SF.stack_gpt_draws([gpt[:3]], 9).shape == (1, 9)
    out = output_path("/in/d/e/clip.npy", "/out", "/in", "flac")
    assert SF.output_stem(out, "/out") == "d/e/clip" and SF.output_stem(output_path("/in/d/clip.npy", "/out", None), "/out") == "clip"


def test_reading_semantic_files(tmp_path):
    ids = (np.arange(12) * 5) % 100
    for k, a in enumerate((ids.astype(np.int16), ids.astype(np.int64)[None], ids.astype(np.int64)[None, None])):
        np.save(tmp_path / f"ok{k}.npy", a)
        got = SF.read_semantic_file(tmp_path / f"ok{k}.npy", 100)
        assert got.dtype == np.int64 and got.shape == (12,) and np.array_equal(got, ids)
    cases = {"float": (ids.astype(np.float32), "dtype"), "int32": (ids.astype(np.int32), "dtype"), "rank": (np.zeros((2, 6), dtype=np.int64), "rank 2"),
             "rank4": (np.zeros((1, 1, 1, 6), dtype=np.int64), "rank 4"), "empty": (np.zeros((1, 0), dtype=np.int64), "empty"),
             "long": (np.zeros(65537, dtype=np.int16), "65537"), "past": (np.array([1, 100], dtype=np.int64), "100 outside"),
             "negative": (np.array([-1, 5], dtype=np.int16), "-1 outside")}
    for name, (a, text) in cases.items():
        np.save(tmp_path / f"{name}.npy", a)
        with pytest.raises(TokenFileError, match=text):
            SF.read_semantic_file(tmp_path / f"{name}.npy", 100)
    (tmp_path / "junk.npy").write_bytes(b"not a numpy file")
    with pytest.raises(TokenFileError, match="unreadable"):
        SF.read_semantic_file(tmp_path / "junk.npy", 100)
    with pytest.raises(TokenFileError, match="unreadable"):
        SF.read_semantic_file(tmp_path / "missing.npy", 100)
    np.save(tmp_path / "most.npy", np.zeros(65536, dtype=np.int16))
    assert SF.read_semantic_file(tmp_path / "most.npy", 100).shape == (65536,)


class StubTok:
    device = "cpu"
    num_codebooks = 8

    def __init__(self):
        self.skipped_files = []


class StubDecoder:
    """[B, 8, T] codes -> [B, 1, 320 T] floats that name their codes: sample t of a frame is code book 0's id / 2048."""
    def forward(self, toks):
        return (toks[:, 0].clamp(min=0).float() / 2048.0).repeat_interleave(320, dim=1).unsqueeze(1)


class StubStages:
    """A source of N ids becomes N + 1 frames whose code book c holds id + c; a source that starts with 99 produces no whole frame."""
    def __init__(self):
        self.calls = []

    def __call__(self, sources, stems):
        self.calls.append(list(stems))
        codes = [None if s[0] == 99 else np.stack([np.concatenate([s, s[-1:]]) + c for c in range(8)]) for s in sources]
        return codes, {"gpt_ticks": 10, "fine_passes": 2, "gpt_s": 0.5, "fine_s": 0.25}


def run_stub(tmp_path, round_files, **kw):
    tree, out, codes = tmp_path / "tree", tmp_path / f"out{round_files}", tmp_path / f"codes{round_files}"
    if not tree.exists():
        os.makedirs(tree / "d")
        for i in range(7):
            np.save(tree / ("d" if i % 2 else "") / f"s{i}.npy", (np.arange(8 + i) + i).astype(np.int16))
        np.save(tree / "bad_dtype.npy", np.zeros(4, dtype=np.float64))
        np.save(tree / "d" / "noframe.npy", np.array([99, 1, 2], dtype=np.int64))
        np.save(tree / "d" / "past.npy", np.array([1, 200], dtype=np.int64))
    tok, stages = StubTok(), StubStages()
    files = sorted(str(p) for p in tree.rglob("*.npy"))
    inputs = [(f, output_path(f, str(out), str(tree), "wav")) for f in files]
    SF.to_audio_files(tok, StubDecoder(), inputs, str(out), stages, 100, round_files, str(codes), 2, kw.get("chunk_size"), 2, False, False, 1 << 30, 24000, 75,
                      "wav", False, log=RunLog(tok, "to_audio_batch_files", "audio"))
    return tok, stages, out, codes


def test_round_planning_and_skips_against_a_stub(tmp_path):
    tok, stages, out, codes = run_stub(tmp_path, 3)
    valid = ["d/noframe", "d/s1", "d/s3", "d/s5", "s0", "s2", "s4", "s6"]      # in walking order, as read_semantic_file accepts them
    assert stages.calls == [valid[0:3], valid[3:6], valid[6:8]], "rounds of round_files VALID files, in order, keyed by the relative output stem"
    reasons = {os.path.basename(p): why for p, why in tok.skipped_files}
    assert sorted(reasons) == ["bad_dtype.npy", "noframe.npy", "past.npy"]
    assert "dtype" in reasons["bad_dtype.npy"] and "outside" in reasons["past.npy"] and reasons["noframe.npy"] == SF.NO_FRAME
    s = tok.run_summary
    assert (s["rounds"], s["gpt_ticks"], s["fine_passes"], s["files"], s["skipped_files"]) == (3, 30, 6, 7, 3)
    assert s["generated_frames"] == sum(8 + i + 1 for i in range(7)) and tok.run_timings["gpt_s"] == 1.5 and tok.run_timings["fine_s"] == 0.75
    for i in range(7):
        stem = ("d/" if i % 2 else "") + f"s{i}"
        c = np.load(codes / (stem + ".npy"))
        assert c.dtype == np.int16 and c.shape == (8, 9 + i) and c[3, 0] == i + 3
        assert os.path.getsize(out / (stem + ".wav")) == 44 + 2 * 320 * (9 + i)
    assert not (out / "d" / "noframe.wav").exists() and not (codes / "d" / "noframe.npy").exists()
    # another round size: other rounds, the same files
    tok2, stages2, out2, _ = run_stub(tmp_path, 8, chunk_size=0.05)
    assert stages2.calls == [valid] and tok2.run_summary["rounds"] == 1 and tok2.run_summary["files"] == 7
    for i in range(7):
        stem = ("d/" if i % 2 else "") + f"s{i}"
        assert (out2 / (stem + ".wav")).read_bytes() == (out / (stem + ".wav")).read_bytes()
    for bad in (0, 4097):
        with pytest.raises(ValueError, match="round_files"):
            run_stub(tmp_path, bad)


def test_interface_refusals(tmp_path):
    np.save(tmp_path / "s.npy", np.arange(5))
    with pytest.raises(ValueError, match="decode_batch_files"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_audio_batch_files(2, tmp_path / "out", token_dir=tmp_path)
    for tok in (Tokenizers.semantic_m, Tokenizers.semantic_s):
        at = AudioToken(tok, device="cuda:0")
        with pytest.raises(ValueError, match="audio_format"):
            at.to_audio_batch_files(2, tmp_path / "out", token_dir=tmp_path, audio_format="mp3")
        for kw in (dict(slots=0), dict(slots=65), dict(fine_slots=0), dict(fine_slots=65), dict(round_files=0), dict(round_files=4097)):
            with pytest.raises(ValueError, match=next(iter(kw))):
                at.to_audio_batch_files(2, tmp_path / "out", token_dir=tmp_path, **kw)
        assert getattr(at, "semantic_decoder", None) is None and getattr(at, "fine_decoder", None) is None, "refused before any model is built"
        with pytest.raises(NotImplementedError):
            at.decode_batch_files(2, tmp_path / "out", token_dir=tmp_path)
        with pytest.raises(NotImplementedError):
            at.load_decoder()
    with pytest.raises(ValueError, match="audio_format"):
        AudioToken(Tokenizers.acoustic, device="cuda:0").to_audio_batch_files(2, tmp_path / "out", token_dir=tmp_path, audio_format="mp3")
    assert not (tmp_path / "out").exists()
