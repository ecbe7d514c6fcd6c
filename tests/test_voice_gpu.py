"""GPU: voice prompts through the public interface: ``to_audio(long_form=True, voice=)`` against the three stages composed by hand, with and
without ``slots=``; ``to_audio_batch_files(voice=)`` against the hand-written ``to_audio`` loop over its rounds; ``voice_prompt(path)`` on the synthetic
models. The models are tests/test_semantic_files_gpu.py's: a 2-layer synthetic GPT at ``window=8, hop=4`` and fine model "a" of tests/fine_cases.py."""
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from audiotoken_amd import AudioToken, Tokenizers
from audiotoken_amd import semantic_files as SF
from audiotoken_amd import weights as W
from audiotoken_amd.configs import HubertDecoderConfig, Wav2VecBertDecoderConfig
from audiotoken_amd.fine_decoder import fine_windows, history_cells
from audiotoken_amd.fine_decoder import seeded_uniforms as fine_uniforms
from audiotoken_amd.semantic_decoder import seeded_uniforms
from audiotoken_amd.voice import VoicePrompt

from tests import fine_cases
from tests.test_semantic_files_gpu import read_all

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


def tokenizer():
    if "sem" not in _cache:
        gpt = W.synth_gpt_weights(n_layer=2, vocab=Wav2VecBertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
        _cache["sem"] = AudioToken(Tokenizers.semantic_m, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))
        _cache["ac"] = AudioToken(Tokenizers.acoustic, device=DEV, num_codebooks=8)
    return _cache["sem"], _cache["ac"]


def voice(P=4, seed=0):
    g = np.random.default_rng(31 + seed)
    return VoicePrompt(g.integers(0, 1000, size=P), g.integers(0, 1024, size=(8, 3 * P // 2)))


def source(i):
    return ((np.arange(9 + (5 * i) % 9) * 7 + i) % 1000).astype(np.int64)


@pytest.mark.parametrize("slots", [None, 2])
def test_to_audio_with_a_voice_is_the_three_stages_composed(slots):
    sem, ac = tokenizer()
    a, b = voice(4, 0), voice(2, 1)
    srcs, voices = [source(0), source(3), source(6)], [a, None, b]
    kw = dict(long_form=True, window=8, hop=4, max_new_tokens=12, **({} if slots is None else {"slots": slots}))
    u1 = seeded_uniforms(21, 3, 80)
    coarse_by_hand = sem.to_acoustic(srcs, uniforms=u1, voice=voices, **kw)
    assert [w[0][2] for w in coarse_by_hand.windows] == [12, 0, 6], "window 0 carries the prompt's 3 P coarse ids"
    hists = [a.codes, None, b.codes]
    n_max = max(len(fine_windows(int(c.shape[1]), 128, 0 if h is None else history_cells(int(h.shape[1]), 128))) for c, h in zip(coarse_by_hand.codes, hists))
    u2 = fine_uniforms(22, 3, n_max, 128)
    fine_by_hand = sem.to_fine(coarse_by_hand.codes, uniforms=u2, history=hists)
    audio, coarse, fine = sem.to_audio(srcs, uniforms=u1, fine_uniforms=u2, voice=voices, **kw)
    plain = sem.to_acoustic(srcs, uniforms=u1, **kw)
    for i in range(3):
        T = coarse_by_hand.codes[i].shape[1]
        assert torch.equal(coarse.ids[i], coarse_by_hand.ids[i]) and coarse.windows == coarse_by_hand.windows
        assert torch.equal(fine.codes[i], fine_by_hand.codes[i]) and torch.equal(fine.codes[i][:2], coarse.codes[i]) and fine.codes[i].shape == (8, T)
        want = ac.decode(fine_by_hand.codes[i].unsqueeze(0))
        assert audio[i].shape == (1, 320 * T), "the audio covers the generated frames only"
        assert torch.equal(audio[i], want), "bit-equal to the three stages composed by hand"
    assert not torch.equal(plain.ids[0], coarse.ids[0]) and not torch.equal(plain.ids[2], coarse.ids[2]), "a prompt changes what is generated"
    with pytest.raises(ValueError, match="8 code books"):
        sem.to_audio(srcs, voice=VoicePrompt(np.arange(2), np.zeros((2, 3), dtype=np.int64)), **kw)


def test_to_audio_batch_files_with_a_voice_is_the_to_audio_loop(tmp_path):
    sem, ac = tokenizer()
    v = voice(4, 2)
    names = ["a/s0", "a/s1", "b/s2", "b/s3", "b/s4"]
    tree, out, codes_dir = str(tmp_path / "tree"), str(tmp_path / "out"), str(tmp_path / "codes")
    for i, n in enumerate(names):
        os.makedirs(os.path.dirname(os.path.join(tree, n)), exist_ok=True)
        np.save(os.path.join(tree, n + ".npy"), source(i))
    gen = dict(window=8, hop=4, max_new_tokens=12, slots=4, fine_slots=2, seed=9)
    sem.to_audio_batch_files(2, out, token_dir=tree, round_files=3, codes_dir=codes_dir, voice=v, **gen)
    assert sem.run_summary["files"] == 5 and sem.run_summary["rounds"] == 2 and not sem.skipped_files
    stages = SF.Stages(sem, 9, 0.8, 100, 0.5, 12, 8, 4, 4, 2, voice=v)
    h = history_cells(v.frames, 128)
    saved = {}
    for at in (0, 3):   # the hand-written loop: one to_audio call per round, with each file's own draws
        part = names[at:at + 3]
        srcs = [source(names.index(n)) for n in part]
        caps = [stages.capacity(len(s)) for s in srcs]
        u = SF.stack_gpt_draws([SF.file_draws(9, n, cap)[0] for n, cap in zip(part, caps)])
        coarse = sem.to_acoustic(srcs, long_form=True, window=8, hop=4, max_new_tokens=12, slots=4, uniforms=u, voice=v)
        n_win = [len(fine_windows(int(c.shape[1]), 128, h)) for c in coarse.codes]
        fu = np.zeros((len(part), max(n_win), 6, 128), dtype=np.float32)
        for i, (n, cap) in enumerate(zip(part, caps)):
            fu[i, :n_win[i]] = SF.file_draws(9, n, cap, n_win[i], 128)[1]
        audio, coarse2, fine = sem.to_audio(srcs, long_form=True, window=8, hop=4, max_new_tokens=12, slots=4, uniforms=u, fine_uniforms=fu, voice=v)
        for i, n in enumerate(part):
            got = torch.from_numpy(np.load(os.path.join(codes_dir, n + ".npy")).astype(np.int64))
            assert torch.equal(got, fine.codes[i]), f"{n}: the file's codes are the to_audio loop's"
            assert audio[i].shape == (1, 320 * got.shape[1])
            saved[n] = got
    want_dir = str(tmp_path / "want")
    ac.decode_batch_files(2, want_dir, token_dir=codes_dir, chunk_size=None)
    got_wav, want_wav = read_all(out, ".wav"), read_all(want_dir, ".wav")
    assert sorted(got_wav) == sorted(names) == sorted(want_wav)
    for n in names:
        assert got_wav[n] == want_wav[n] and len(got_wav[n]) == 44 + 2 * 320 * saved[n].shape[1]
    plain_dir = str(tmp_path / "plain")
    sem.to_audio_batch_files(2, plain_dir, token_dir=tree, round_files=3, **gen)
    assert any(read_all(plain_dir, ".wav")[n] != got_wav[n] for n in names), "the prompt changes the audio"
    with pytest.raises(ValueError):
        sem.to_audio_batch_files(2, out, token_dir=tree, voice=voice(6), **gen)   # longer than window - hop: refused before a file is read


def test_voice_prompt_from_a_file(tmp_path):
    from scipy.io import wavfile
    gpt = W.synth_gpt_weights(n_layer=2, vocab=HubertDecoderConfig().VOCAB_SIZE, block=1024, seed=0, family="peaky")
    sem = AudioToken(Tokenizers.semantic_s, device=DEV, decoder_weights=gpt, fine_weights=fine_cases.weights("a", "peaky"))
    path = Path(tmp_path / "clip.wav")
    wav = W.synth_waveform(1, 32000, 16000, seed=3)[0]
    wavfile.write(str(path), 16000, np.clip(wav * 32767, -32768, 32767).astype(np.int16))
    v = sem.voice_prompt(path)
    assert isinstance(v, VoicePrompt) and len(v) % 2 == 0 and 2 <= len(v) <= 128 and v.codes.shape == (8, 3 * len(v) // 2)
    assert len(v) >= 90, "2 s of audio: about 100 ids and 150 frames, all of it below the default limit of window - hop"
    small = sem.voice_prompt(path, max_ids=4)
    assert len(small) == 4 and small.codes.shape == (8, 6)
    assert torch.equal(small.semantic, v.semantic[-4:]) and torch.equal(small.codes, v.codes[:, -6:]), "the latest aligned stretch"
    src = (np.arange(11) * 5) % 1000
    audio, coarse, fine = sem.to_audio(src, long_form=True, window=8, hop=4, max_new_tokens=12, voice=small)
    T = fine.codes[0].shape[1]
    assert coarse.windows[0][0][2] == 12 and audio[0].shape == (1, 320 * T) and T >= 1
    # the whole prompt at the default window (254, 126): one window of 11 + len(v) ids that carries the prompt's 3 len(v) coarse ids
    coarse = sem.to_acoustic(src, long_form=True, max_new_tokens=12, voice=v)
    assert coarse.windows[0][0][:3] == (0, 11 + len(v), 3 * len(v)) and len(coarse.windows[0]) == 1 and len(coarse.ids[0]) <= 12
