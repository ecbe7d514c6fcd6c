"""GPU: decode_batch_files (audiotoken_amd/writer.py) and the device PCM writer (csrc/pcm_writer.hip: at_pcm_peaks / at_pcm_pack).

What is asserted, and against what:
1. the two kernels against the numpy restatement of the quantisation rule (tests/pcm_ref.py): EQUAL, element for element and count for count;
2. the file pipeline in clamp mode against the existing one-shot decoder (AcousticDecoder.forward on the same padded batches) + the restatement: EQUAL.
   With these synthetic weights the waveform has peak ~6 and about half of the samples lie beyond +-0.99, so this case exercises the clamp heavily and says
   nothing about closeness to the oracle;
3. the file pipeline with rescale=True against the CPU oracle (oracle/encodec_ref.acoustic_decode of every segment ALONE and UNPADDED, concatenated,
   rescaled by the oracle's own file peak p_o): the decode bar of this project is max-abs < 1e-3 (tests/parity.FLOAT_TOL); with both peaks >= 0.99 the two
   scaled waveforms differ by at most 2 * 0.99 * 1e-3 / p_o, so per file max |pcm - pcm_oracle| <= floor(32768 * 2 * 0.99 * FLOAT_TOL / p_o) + 1, computed
   from the oracle's peak (about 12 LSB at p_o ~ 6). This also shows that right padding is harmless on the device;
4. the round trip encode_batch_files -> decode_batch_files -> encode_batch_files on a small WAV corpus (paths, lengths, readability);
5. robustness: bad files among good ones, and device_writer=False writing the same bytes.
"""
import ctypes as C
import os
import wave

import numpy as np
import pytest
import torch

from audiotoken_amd import audio_io as A
from audiotoken_amd import prng
from audiotoken_amd import weights as W
from audiotoken_amd import writer as Wr
from oracle import encodec_ref as R
from tests import pcm_ref as P
from tests.parity import FLOAT_TOL

pytestmark = pytest.mark.gpu
HOP = 320
CHUNK_S, CHUNK_FRAMES = 0.4, 30          # 0.4 s = 30 frames per row: the CPU oracle takes seconds


@pytest.fixture(scope="module")
def weights():
    return W.synth_encodec_weights(seed=0, with_decoder=True)


@pytest.fixture(scope="module")
def tok(cuda_device, weights):
    from audiotoken_amd import AudioToken, Tokenizers
    return AudioToken(Tokenizers.acoustic, device="cuda:0", num_codebooks=8, weights=weights)


def _codes(name, K, T):
    return np.minimum((prng.uniform01(f"decode_files|{name}", K * T, 0) * np.float32(1024.0)).astype(np.int64), 1023).reshape(K, T)


TREE = {"a.npy": (8, 3 * CHUNK_FRAMES + 11),      # several chunks plus a short tail
        "b.npy": (8, 4),                          # below the decoder's 7 frames
        "c.npy": (2, 40),                         # K = 2 between files of K = 8
        "d.npy": (8, 30),
        "sub/e.npy": (8, 45)}                     # in a sub-directory


@pytest.fixture(scope="module")
def token_tree(tmp_path_factory):
    root = tmp_path_factory.mktemp("tokens")
    (root / "sub").mkdir()
    toks = {}
    for name, (K, T) in TREE.items():
        toks[name] = _codes(name, K, T)
        np.save(root / name, toks[name].astype(np.int16) if name == "d.npy" else (toks[name][None] if name == "c.npy" else toks[name]))
    return root, toks


def _read(path):
    with wave.open(str(path), "rb") as f:
        assert (f.getnchannels(), f.getsampwidth(), f.getframerate()) == (1, 2, 24000)
        return np.frombuffer(f.readframes(f.getnframes()), dtype="<i2")


def _wav_name(name):
    return name[:-4] + ".wav"


# ---- 1. the kernels against the restatement, exact --------------------------------------------------------------------------------------------------------------
def _kernel_rows(rows, src_np, limit=0.99):
    """rows = [(src_off, dst_off, n, scale)] -> (packed int16 [dst_len] with sentinel gaps, peaks, counts) from the device."""
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    dev = torch.device("cuda:0")
    dst_len = max([d + n for _, d, n, _ in rows] + [0]) + 64
    src = torch.from_numpy(src_np).to(dev)
    dst = torch.full((dst_len,), 0x7777, dtype=torch.int16, device=dev)
    descs = (_cabi.PcmRowDesc * len(rows))(*[_cabi.PcmRowDesc(s, d, n, sc, 0) for s, d, n, sc in rows])
    descs_dev = torch.from_numpy(np.frombuffer(descs, dtype=np.uint8).copy()).to(dev)
    peaks = torch.full((len(rows),), -1.0, dtype=torch.float32, device=dev)
    counts = torch.full((len(rows), 2), -1, dtype=torch.int32, device=dev)
    max_n = max(r[2] for r in rows)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(lib.at_pcm_peaks(src.data_ptr(), descs_dev.data_ptr(), len(rows), max_n, peaks.data_ptr(), stream), "at_pcm_peaks")
    _cabi.check(lib.at_pcm_pack(src.data_ptr(), descs_dev.data_ptr(), len(rows), max_n, limit, dst.data_ptr(), counts.data_ptr(), stream), "at_pcm_pack")
    torch.cuda.synchronize()
    return dst.cpu().numpy(), peaks.cpu().numpy(), counts.cpu().numpy().view(np.uint32)


def _hard_values(n, seed):
    """Mostly N(0, 0.7) (a third beyond +-0.99 after scaling), with exact half-way cases, the limits, huge values, NaN and +-inf sprinkled in."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.7).astype(np.float32)
    k = rng.integers(-32000, 32000, size=n).astype(np.float32)
    halves = (k + np.float32(0.5)) / np.float32(32768.0)
    pick = rng.random(n)
    x = np.where(pick < 0.15, halves, x)
    special = np.array([np.nan, np.inf, -np.inf, 0.99, -0.99, 1.0, -1.0, 3.0e38, -3.0e38, -0.0, 1e-42, 6.0, -6.0], dtype=np.float32)
    at = rng.random(n) < 0.02
    x[at] = special[rng.integers(0, len(special), size=int(at.sum()))]
    return x.astype(np.float32)


def _check_against_restatement(rows, src_np):
    dst, peaks, counts = _kernel_rows(rows, src_np)
    covered = np.zeros(len(dst), dtype=bool)
    for i, (s, d, n, sc) in enumerate(rows):
        x = src_np[s:s + n]
        want, clipped, nonfinite = P.quantise(x, np.float32(sc))
        assert np.array_equal(dst[d:d + n], want), f"row {i} (src_off {s}, dst_off {d}, n {n}, scale {sc})"
        assert (int(counts[i, 0]), int(counts[i, 1])) == (clipped, nonfinite), f"row {i} counts"
        assert peaks[i] == P.peak(x), f"row {i} peak {peaks[i]} vs {P.peak(x)}"
        covered[d:d + n] = True
    assert np.all(dst[~covered] == 0x7777), "the pack wrote outside its rows"


def test_kernels_equal_the_restatement_on_ragged_rows(cuda_device):
    """Seven rows: aligned and misaligned source / destination offsets, lengths that are no multiple of the 8-sample group or the 2048-sample tile, one
    exact tile, a single sample, an empty row, a row of only non-finite samples; scales below, at and above 1."""
    lens = [5003, 2048, 1, 4096 + 8, 0, 777, 320 * 9]
    src_offs, dst_offs, pos_s, pos_d = [], [], 0, 0
    for i, n in enumerate(lens):
        pos_s += (0, 3, 0, 5, 0, 1, 0)[i]            # misalign some sources (floats) ...
        pos_d += (0, 0, 8, 1, 0, 3, 5)[i]            # ... and some destinations (int16), leaving gaps the pack must not touch
        src_offs.append(pos_s); dst_offs.append(pos_d)
        pos_s += (n + 7) // 8 * 8
        pos_d += (n + 7) // 8 * 8
    src = _hard_values(pos_s + 16, 1)
    src[src_offs[5]:src_offs[5] + 777] = np.where(np.arange(777) % 3 == 0, np.nan, np.where(np.arange(777) % 3 == 1, np.inf, -np.inf))
    scales = [1.0, 0.1640625, 1.0, float(np.float32(0.99) / np.float32(6.01)), 1.0, 1.0, 2.5]
    rows = [(src_offs[i], dst_offs[i], lens[i], scales[i]) for i in range(len(lens))]
    _check_against_restatement(rows, src)


def test_kernels_equal_the_restatement_on_decoder_shaped_batches(cuda_device):
    """The product's shapes: rows at multiples of 320 * T_max (the vector path), ragged valid lengths, compacted output; 3 rows and 70 rows."""
    for B, t_max, seed in ((3, 60, 2), (70, 33, 3)):
        rng = np.random.default_rng(seed)
        valid = rng.integers(1, t_max + 1, size=B)
        valid[0] = t_max
        src = _hard_values(B * HOP * t_max, seed + 10)
        rows, pos = [], 0
        for b in range(B):
            rows.append((b * HOP * t_max, pos, HOP * int(valid[b]), float(np.float32(rng.uniform(0.1, 1.0)))))
            pos += HOP * int(valid[b])
        _check_against_restatement(rows, src)


def test_kernels_take_more_tiles_than_the_grid(cuda_device):
    """2300 short rows: more tiles than the launch has workgroups, so every workgroup walks several rows grid-stride."""
    rng = np.random.default_rng(5)
    lens = rng.integers(1, 90, size=2300)
    src = _hard_values(int(lens.sum()) + 8, 6)
    rows, pos = [], 0
    for n in lens:
        rows.append((pos, pos, int(n), 1.0))
        pos += int(n)
    _check_against_restatement(rows, src)


def test_entry_points_validate_before_touching_the_device(cuda_device):
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    x = torch.zeros(64, device="cuda:0")
    p = x.data_ptr()
    assert lib.at_pcm_pack(None, p, 1, 8, 0.99, p, p, None) != 0 and "at_pcm_pack" in _cabi.last_error()
    assert lib.at_pcm_pack(p, p, -1, 8, 0.99, p, p, None) != 0
    assert lib.at_pcm_pack(p, p, 1, -8, 0.99, p, p, None) != 0
    assert lib.at_pcm_pack(p, p, 1, 8, 1.5, p, p, None) != 0 and "limit" in _cabi.last_error()
    assert lib.at_pcm_peaks(p, None, 1, 8, p, None) != 0 and "at_pcm_peaks" in _cabi.last_error()
    assert lib.at_pcm_peaks(p, p, 1, -1, p, None) != 0
    assert lib.at_pcm_pack(p, p, 0, 0, 0.99, p, p, None) == 0 and lib.at_pcm_peaks(p, p, 0, 0, p, None) == 0
    torch.cuda.synchronize()


# ---- 2. end to end, clamp mode, exact against the existing decoder ----------------------------------------------------------------------------------------------
def _plans(toks):
    order = sorted(toks)          # the walk's order: a, b, c, d, sub/e
    return order, list(Wr.plan_batches([(i, *toks[n].shape) for i, n in enumerate(order)], batch_size=4, chunk_frames=CHUNK_FRAMES))


def test_clamp_mode_equals_the_one_shot_decoder(tok, token_tree, tmp_path):
    root, toks = token_tree
    out = tmp_path / "wav"
    tok.decode_batch_files(batch_size=4, outdir=out, chunk_size=CHUNK_S, num_workers=2, token_dir=root)
    assert tok.skipped_files == []
    order, plans = _plans(toks)
    assert any(p.K == 2 for p in plans) and any(p.t_max == 7 for p in plans) and len(plans) >= 4
    want = {n: [] for n in order}
    clipped = nonfinite = 0
    for plan in plans:
        batch = Wr.padded_tokens(plan, lambda i: toks[order[i]])
        wav = tok.decoder.forward(batch.cuda())                   # existing code, the same padded batch
        assert tok.decoder.last_status() == 0
        wav = wav.reshape(len(plan.rows), HOP * plan.t_max).cpu().numpy()
        for b, r in enumerate(plan.rows):
            q, c, nf = P.quantise(wav[b, :HOP * r.valid])
            want[order[r.file]].append(q)
            clipped += c
            nonfinite += nf
    n_clamped = 0
    for name in order:
        got = _read(out / _wav_name(name))
        ref = np.concatenate(want[name])
        assert len(got) == HOP * toks[name].shape[1]
        assert np.array_equal(got, ref), f"{name}: {int((got != ref).sum())} of {len(ref)} samples differ"
        n_clamped += int((np.abs(got.astype(np.int32)) == 32440).sum())
    s = tok.run_summary
    print(f"clamp mode: {clipped} clipped samples of {sum(HOP * t.shape[1] for t in toks.values())}, {n_clamped} at the limit")
    assert s["clipped_samples"] == clipped and s["nonfinite_samples"] == nonfinite == 0
    assert (s["files"], s["segments"], s["batches"], s["skipped_files"]) == (5, sum(len(p.rows) for p in plans), len(plans), 0)
    assert clipped > 1000                                         # the case exercises the clamp


# ---- 3. end to end, rescale=True, against the CPU oracle --------------------------------------------------------------------------------------------------------
def test_rescale_mode_is_within_the_decode_bar_of_the_oracle(tok, token_tree, weights, tmp_path):
    root, toks = token_tree
    out = tmp_path / "wav"
    tok.decode_batch_files(batch_size=4, outdir=out, chunk_size=CHUNK_S, num_workers=0, token_dir=root, rescale=True)
    assert tok.skipped_files == []
    for name, t in toks.items():
        parts = [R.acoustic_decode(weights, torch.from_numpy(t[None, :, t0:t0 + CHUNK_FRAMES])).numpy().ravel()      # every segment alone, unpadded
                 for t0 in range(0, t.shape[1], CHUNK_FRAMES)]
        x = np.concatenate(parts).astype(np.float32)
        p_o = P.peak(x)
        assert p_o >= 0.99, f"{name}: the bound below assumes both peaks >= 0.99 (oracle peak {p_o})"
        ref, _, _ = P.quantise(x, P.file_scale(p_o))
        got = _read(out / _wav_name(name))
        assert len(got) == len(ref) == HOP * t.shape[1]
        bound = int(np.floor(32768.0 * 2.0 * 0.99 * FLOAT_TOL / float(p_o))) + 1
        err = int(np.abs(got.astype(np.int32) - ref.astype(np.int32)).max())
        print(f"{name}: oracle peak {float(p_o):.3f}, max |pcm - pcm_oracle| {err} LSB, bound {bound} LSB, device peak code {int(np.abs(got.astype(np.int32)).max())}")
        assert err <= bound, f"{name}: {err} LSB > {bound} LSB"
    assert tok.run_summary["files"] == 5 and tok.run_summary["nonfinite_samples"] == 0


# ---- 4. round trip ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_round_trip_encode_decode_encode(tok, tmp_path):
    from scipy.io import wavfile
    src, tokdir, out, tokdir2 = tmp_path / "audio", tmp_path / "tokens", tmp_path / "decoded", tmp_path / "tokens2"
    (src / "spk" / "x").mkdir(parents=True)
    sr, c = 24000, 1
    lens = {"one.wav": int(2.3 * sr), "two.wav": sr, "spk/three.wav": int(1.5 * sr) + 123, "spk/x/four.wav": int(0.4 * sr)}
    for i, (name, n) in enumerate(lens.items()):
        wavfile.write(str(src / name), sr, np.round(W.synth_waveform(1, n, sr, seed=900 + i)[0] * 20000).astype(np.int16))
    tok.encode_batch_files(batch_size=3, outdir=tokdir, chunk_size=c, num_workers=2, audio_dir=src)
    assert tok.skipped_files == []
    tok.decode_batch_files(batch_size=3, outdir=out, chunk_size=c, num_workers=2, token_dir=tokdir)
    assert tok.skipped_files == [] and tok.run_summary["files"] == len(lens)
    for name, n in lens.items():
        t = np.load(tokdir / (name[:-4] + ".npy"))
        T_file = t.shape[-1]
        assert t.shape[0] == 8 and T_file >= n // HOP
        path = out / name                                         # the mirrored relative path
        assert path.exists(), name
        assert len(_read(path)) == HOP * T_file
        back = A.read_audio(str(path), sr)
        assert back.shape == (1, HOP * T_file) and bool(torch.isfinite(back).all()) and float(back.abs().max()) <= 0.99 + 1e-6
    tok.encode_batch_files(batch_size=3, outdir=tokdir2, chunk_size=c, num_workers=0, audio_dir=out)      # the outputs are inputs again
    assert tok.skipped_files == []
    for name in lens:
        assert np.load(tokdir2 / (name[:-4] + ".npy")).shape == np.load(tokdir / (name[:-4] + ".npy")).shape


# ---- 5. robustness ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_bad_files_are_skipped_and_the_good_ones_written(tok, token_tree, tmp_path):
    root, toks = token_tree
    src, out = tmp_path / "t", tmp_path / "o"
    src.mkdir()
    np.save(src / "a_good.npy", toks["d.npy"])
    (src / "b_corrupt.npy").write_bytes(b"\x93NUMPY\x01\x00 this header never ends")
    bad = toks["a.npy"].copy()
    bad[5, 17] = 1024
    np.save(src / "c_range.npy", bad)
    np.save(src / "d_good.npy", toks["sub/e.npy"])
    tok.decode_batch_files(batch_size=4, outdir=out, chunk_size=CHUNK_S, num_workers=2, token_dir=src)
    assert sorted(os.listdir(out)) == ["a_good.wav", "d_good.wav"]
    reasons = {os.path.basename(p): why for p, why in tok.skipped_files}
    assert sorted(reasons) == ["b_corrupt.npy", "c_range.npy"]
    assert "unreadable token file" in reasons["b_corrupt.npy"] and "code 1024 outside [0, 1023]" in reasons["c_range.npy"]
    s = tok.run_summary
    assert (s["files"], s["skipped_files"], s["segments"]) == (2, 2, 1 + 2)
    assert len(_read(out / "a_good.wav")) == HOP * 30 and len(_read(out / "d_good.wav")) == HOP * 45


@pytest.mark.parametrize("rescale", [False, True])
def test_host_conversion_path_writes_the_same_bytes(tok, token_tree, tmp_path, rescale):
    root, toks = token_tree
    dev_out, host_out = tmp_path / "dev", tmp_path / "host"
    tok.decode_batch_files(batch_size=3, outdir=dev_out, chunk_size=CHUNK_S, num_workers=0, token_dir=root, rescale=rescale)
    dev_summary = dict(tok.run_summary)
    tok.decode_batch_files(batch_size=3, outdir=host_out, chunk_size=CHUNK_S, num_workers=0, token_dir=root, rescale=rescale, device_writer=False)
    for name in toks:
        a, b = (dev_out / _wav_name(name)).read_bytes(), (host_out / _wav_name(name)).read_bytes()
        assert len(a) == 44 + 2 * HOP * toks[name].shape[1] and a == b, name
    assert dev_summary == tok.run_summary
    assert tok.run_timings["bytes_downloaded"] > 0
