"""GPU: the device FLAC encoder (csrc/flac_encode.hip: at_flac_encode_rows) and decode_batch_files(audio_format="flac").

What is asserted, and against what:
1. the kernel against the numpy restatement of the rule (tests/flac_enc_ref.py on the samples of tests/pcm_ref.py): block records, compacted subframe bytes
   and per-row counts EQUAL, and the sentinel bytes beyond the total untouched;
2. the entry point validates its arguments before the device is touched;
3. the file pipeline on the token tree of test_decode_files_gpu.py, in clamp and in rescale mode: every .flac decodes, through the package's own reader, to
   exactly the int16 samples of the .wav that audio_format="wav" writes from the same tokens; the relative tree is kept; bad files are skipped and recorded;
   device_writer=False writes identical bytes; every file is at most 42 + sum over its blocks of (2 n + 17) bytes (a VERBATIM subframe is 1 + 2 n bytes, a
   frame adds at most 14 header bytes and 2 of CRC-16: derived, not measured);
4. round trip: encode_batch_files on the FLAC tree returns the tokens it returns on the WAV tree, EQUAL;
5. save_audio of a device tensor writes the restatement's file.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from audiotoken_amd import audio_io as A
from tests import flac_enc_ref as F
from tests import pcm_ref as P
from tests.test_decode_files_gpu import CHUNK_S, TREE, _hard_values, _read, tok, token_tree, weights  # noqa: F401 — the same token tree and tokenizer

pytestmark = pytest.mark.gpu
HOP = 320
SENTINEL = 0x77


# ---- 1. the kernel against the restatement, exact ---------------------------------------------------------------------------------------------------------------
def _kernel_rows(rows, src_np, limit=0.99):
    """rows = [(src_off, n, scale)] -> (records, bytes buffer with 64 sentinel bytes of slack, counts, worst-case capacity) from the device."""
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    dev = torch.device("cuda:0")
    descs, nblocks = [], 0
    for s, n, sc in rows:
        descs.append(_cabi.FlacRowDesc(s, n, nblocks, sc))
        nblocks += (n + 4095) // 4096
    cap = nblocks + 2 * sum(n for _, n, _ in rows)
    src = torch.from_numpy(src_np).to(dev)
    arr = (_cabi.FlacRowDesc * len(rows))(*descs)
    descs_dev = torch.from_numpy(np.frombuffer(arr, dtype=np.uint8).copy()).to(dev)
    recs = torch.full((40 * nblocks,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((cap + 64,), SENTINEL, dtype=torch.uint8, device=dev)
    counts = torch.full((len(rows), 2), -1, dtype=torch.int32, device=dev)
    ws_bytes = lib.at_flac_encode_workspace_bytes(nblocks)
    ws = torch.empty(ws_bytes + 16, dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    _cabi.check(lib.at_flac_encode_rows(src.data_ptr(), descs_dev.data_ptr(), len(rows), nblocks, limit, recs.data_ptr(), out.data_ptr(), cap, counts.data_ptr(),
                                        ws.data_ptr(), ws_bytes, stream), "at_flac_encode_rows")
    torch.cuda.synchronize()
    return recs.cpu().numpy().view(_cabi.FLAC_BLOCK_DTYPE), out.cpu().numpy(), counts.cpu().numpy().view(np.uint32), cap


def _check_against_restatement(rows, src_np):
    recs, out, counts, cap = _kernel_rows(rows, src_np)
    want_recs, want_bytes = [], b""
    for i, (s, n, sc) in enumerate(rows):
        q, clipped, nonfinite = P.quantise(src_np[s:s + n], np.float32(sc))
        assert (int(counts[i, 0]), int(counts[i, 1])) == (clipped, nonfinite), f"row {i} counts"
        for a, bn in F.blocks_of(n):
            sub, kind, o, p, _ = F.subframe(q[a:a + bn])
            want_recs.append((a, len(want_bytes), i, bn, kind, o, p, len(sub)))
            want_bytes += sub
    got_recs = [tuple(int(r[f]) for f in ("first", "byte_off", "row", "n", "kind", "order", "porder", "nbytes")) for r in recs]
    for b, (g, w) in enumerate(zip(got_recs, want_recs)):
        assert g == w, f"block {b}: (first, byte_off, row, n, kind, order, porder, nbytes) = {g}, restatement {w}"
    assert len(got_recs) == len(want_recs)
    total = len(want_bytes)
    assert total <= cap
    got = out[:total].tobytes()
    if got != want_bytes:
        at = next(i for i in range(total) if got[i] != want_bytes[i])
        blk = max(b for b, w in enumerate(want_recs) if w[1] <= at)
        raise AssertionError(f"compacted bytes differ first at byte {at}: block {blk} {want_recs[blk]}, byte {at - want_recs[blk][1]} of its subframe")
    assert np.all(out[total:] == SENTINEL), "the encoder wrote beyond the compacted total"
    return want_recs


def test_kernel_equals_the_restatement_on_ragged_rows_of_every_signal(cuda_device):
    """Every signal of the CPU test, and a tone under bursts of noise, at lengths that take every path: CONSTANT / VERBATIM / FIXED 0..4, n <= 32, n = 33 and n
    odd (pmax = 0: a whole wave in one partition), n = 64 (pmax = 1), n = 1408 (pmax = 5: partitions of 44 samples straddle threads), 2240 (partitions of 35),
    whole blocks (pmax = 6), a last block of one sample, an empty row."""
    lens = [4097, 1408, 64, 33, 4095, 2240, 32, 5, 1, 0]
    rows, parts, pos = [], [], 0
    for i, name in enumerate(F.SIGNALS + ("bursts",)):
        for j, n in enumerate(lens[:6] + [lens[6 + i % 4]]):
            rows.append((pos, n, 1.0))
            parts.append(F.as_float(F.bursts(n, j) if name == "bursts" else F.signal(name, n)))
            pad = 3 if j % 2 else 0                          # misalign some rows
            parts.append(np.zeros(pad, np.float32))
            pos += n + pad
    recs = _check_against_restatement(rows, np.concatenate(parts + [np.zeros(8, np.float32)]))
    assert {r[4] for r in recs} == {F.CONSTANT, F.VERBATIM, F.FIXED} and {r[5] for r in recs if r[4] == F.FIXED} == {0, 1, 2, 3, 4}
    assert {0, 1, 5, 6} <= {r[6] for r in recs if r[4] == F.FIXED}


def test_kernel_equals_the_restatement_on_decoder_shaped_rows(cuda_device):
    """Rows of 2240 / 4160 / 9600 samples at multiples of 320 * T_max with scales != 1, over hard values: a third beyond the limit, exact half-way cases,
    NaN and +-infinity."""
    t_max = 30
    src = _hard_values(3 * HOP * t_max, 21)
    rows = [(0, 2240, 0.1640625), (HOP * t_max, 4160, 2.5), (2 * HOP * t_max, 9600, float(np.float32(0.99) / np.float32(6.01)))]
    _check_against_restatement(rows, src)


def test_kernel_equals_the_restatement_on_smooth_rows_with_specials(cuda_device):
    """A 3-row batch of a tone (FIXED of high order, long unary runs where a NaN or an infinity breaks the prediction) with non-finite samples sprinkled in."""
    rng = np.random.default_rng(8)
    n = 4096 + 1408
    src = np.concatenate([F.as_float(F.signal(name, n)) for name in ("sine_a0", "sine_a16", "sine_a256")])
    at = rng.choice(len(src), size=40, replace=False)
    src[at] = np.array([np.nan, np.inf, -np.inf, 3.0e38], np.float32)[rng.integers(0, 4, size=40)]
    _check_against_restatement([(0, n, 1.0), (n, n, 0.5), (2 * n, n, 1.75)], src)


def test_kernel_takes_more_blocks_than_the_grid(cuda_device):
    """2100 rows of 64 samples: more blocks than the launch has workgroups (at most 8 per CU), so workgroups walk several blocks grid-stride."""
    names = ("sine_a16", "uniform_pm3", "silence", "sine_a0", "uniform_full", "spike")
    base = [F.as_float(F.signal(nm, 64 * 350)) for nm in names]
    src = np.concatenate(base)
    rows = [(64 * i, 64, 1.0) for i in range(2100)]
    _check_against_restatement(rows, src)


def test_entry_point_validates_before_touching_the_device(cuda_device):
    from audiotoken_amd import _cabi
    lib = _cabi.load()
    x = torch.zeros(1 << 16, device="cuda:0")
    p = x.data_ptr()
    ws = lib.at_flac_encode_workspace_bytes(2)
    assert ws >= 2 * (1 + 2 * 4096) and lib.at_flac_encode_workspace_bytes(0) == 0
    ok = (p, p, 1, 2, 0.99, p, p, 1 << 14, p, p, ws, None)

    def call(i, v):
        a = list(ok)
        a[i] = v
        return lib.at_flac_encode_rows(*a)
    assert call(0, None) != 0 and "at_flac_encode_rows" in _cabi.last_error()
    assert call(1, None) != 0 and call(5, None) != 0 and call(6, None) != 0 and call(8, None) != 0
    assert call(2, -1) != 0 and call(3, -1) != 0 and call(7, -1) != 0
    assert call(4, 1.5) != 0 and "limit" in _cabi.last_error()
    assert call(10, ws - 1) != 0 and "workspace" in _cabi.last_error()
    assert call(9, None) != 0 and call(9, p + 4) != 0
    assert lib.at_flac_encode_rows(p, p, 0, 1, 0.99, p, p, 64, p, p, ws, None) != 0 and "without rows" in _cabi.last_error()
    assert lib.at_flac_encode_rows(p, p, 0, 0, 0.99, p, p, 0, p, None, 0, None) == 0
    torch.cuda.synchronize()
    assert float(x.abs().max()) == 0.0


# ---- 3. the file pipeline ---------------------------------------------------------------------------------------------------------------------------------------------
def _flac_samples(path):
    raw = A.decode_raw(str(path))                    # the package's own reader: every CRC-8 / CRC-16 verified
    assert raw.sample_rate == 24000 and raw.pcm.shape[0] == 1 and raw.pcm.dtype == np.int16
    return raw.pcm[0]


def _size_bound(n_rows):
    return 42 + sum(2 * bn + 17 for n in n_rows for _, bn in F.blocks_of(n))


@pytest.mark.parametrize("rescale", [False, True])
def test_flac_files_hold_the_samples_of_the_wav_files(tok, token_tree, tmp_path, rescale):
    root, toks = token_tree
    wav_out, flac_out, host_out = tmp_path / "wav", tmp_path / "flac", tmp_path / "host"
    tok.decode_batch_files(batch_size=3, outdir=wav_out, chunk_size=CHUNK_S, num_workers=0, token_dir=root, rescale=rescale)
    wav_summary = dict(tok.run_summary)
    tok.decode_batch_files(batch_size=3, outdir=flac_out, chunk_size=CHUNK_S, num_workers=2, token_dir=root, rescale=rescale, audio_format="flac")
    assert tok.skipped_files == []
    flac_summary = dict(tok.run_summary)
    assert tok.run_timings["bytes_downloaded"] > 0
    tok.decode_batch_files(batch_size=3, outdir=host_out, chunk_size=CHUNK_S, num_workers=0, token_dir=root, rescale=rescale, audio_format="flac",
                           device_writer=False)
    assert dict(tok.run_summary) == flac_summary
    assert {k: v for k, v in flac_summary.items() if k != "audio_bytes"} == {k: v for k, v in wav_summary.items() if k != "audio_bytes"}
    written = sorted(os.path.relpath(os.path.join(d, f), flac_out) for d, _, fs in os.walk(flac_out) for f in fs)
    assert written == sorted(name[:-4] + ".flac" for name in TREE)                       # the relative tree, nothing else (no .part)
    size = 0
    step = HOP * 30
    for name in toks:
        path = flac_out / (name[:-4] + ".flac")
        want = _read(wav_out / (name[:-4] + ".wav"))
        got = _flac_samples(path)
        assert len(got) == HOP * toks[name].shape[1] and np.array_equal(got, want), name
        assert path.read_bytes() == (host_out / (name[:-4] + ".flac")).read_bytes(), name
        rows = [min(step, len(want) - a) for a in range(0, len(want), step)]            # one row per 30-frame segment
        assert os.path.getsize(path) <= _size_bound(rows), name
        assert path.read_bytes() == F.encode_rows([want[a:a + step] for a in range(0, len(want), step)])[0], name
        size += os.path.getsize(path)
    assert flac_summary["audio_bytes"] == size
    assert wav_summary["audio_bytes"] == sum(44 + 2 * HOP * t.shape[1] for t in toks.values())


def test_bad_files_are_skipped_in_flac_mode(tok, token_tree, tmp_path):
    root, toks = token_tree
    src, out = tmp_path / "t", tmp_path / "o"
    src.mkdir()
    np.save(src / "a_good.npy", toks["d.npy"])
    (src / "b_corrupt.npy").write_bytes(b"\x93NUMPY\x01\x00 this header never ends")
    bad = toks["a.npy"].copy()
    bad[5, 17] = 1024
    np.save(src / "c_range.npy", bad)
    np.save(src / "d_good.npy", toks["sub/e.npy"])
    tok.decode_batch_files(batch_size=4, outdir=out, chunk_size=CHUNK_S, num_workers=2, token_dir=src, audio_format="flac")
    assert sorted(os.listdir(out)) == ["a_good.flac", "d_good.flac"]
    reasons = {os.path.basename(p): why for p, why in tok.skipped_files}
    assert sorted(reasons) == ["b_corrupt.npy", "c_range.npy"]
    assert "unreadable token file" in reasons["b_corrupt.npy"] and "code 1024 outside [0, 1023]" in reasons["c_range.npy"]
    s = tok.run_summary
    assert (s["files"], s["skipped_files"], s["segments"]) == (2, 2, 1 + 2)
    assert len(_flac_samples(out / "a_good.flac")) == HOP * 30 and len(_flac_samples(out / "d_good.flac")) == HOP * 45


# ---- 4. round trip ----------------------------------------------------------------------------------------------------------------------------------------------------
def test_tokens_of_the_flac_tree_equal_the_tokens_of_the_wav_tree(tok, token_tree, tmp_path):
    root, toks = token_tree
    outs = {}
    for fmt in ("wav", "flac"):
        tok.decode_batch_files(batch_size=4, outdir=tmp_path / fmt, chunk_size=CHUNK_S, num_workers=0, token_dir=root, audio_format=fmt)
        tok.encode_batch_files(batch_size=3, outdir=tmp_path / (fmt + "_tokens"), chunk_size=1, num_workers=0, audio_dir=tmp_path / fmt)
        assert tok.skipped_files == []
        tokdir = tmp_path / (fmt + "_tokens")
        outs[fmt] = {os.path.relpath(os.path.join(d, f), tokdir): np.load(os.path.join(d, f)) for d, _, fs in os.walk(tokdir) for f in fs}
    # (the encode side skips a segment below its minimum length, as the reference does: the 4-frame file has no token file in either tree)
    assert sorted(outs["flac"]) == sorted(outs["wav"]) and {"a.npy", "c.npy", "d.npy", os.path.join("sub", "e.npy")} <= set(outs["flac"])
    for name in outs["wav"]:
        assert outs["flac"][name].shape[-1] == toks[name.replace(os.sep, "/")].shape[1]
        assert np.array_equal(outs["flac"][name], outs["wav"][name]), name


# ---- 5. save_audio of a device tensor -----------------------------------------------------------------------------------------------------------------------------------
def test_save_audio_of_a_device_tensor(cuda_device, tmp_path):
    x = _hard_values(4096 + 777, 31)
    x[:3000] = F.as_float(F.signal("sine_a16", 3000))
    for rescale in (False, True):
        q, clipped, nonfinite = P.quantise(x, P.file_scale(P.peak(x)) if rescale else np.float32(1.0))
        assert A.save_audio(torch.from_numpy(x).cuda()[None], tmp_path / "x.flac", 24000, rescale=rescale) == (clipped, nonfinite)
        assert (tmp_path / "x.flac").read_bytes() == F.encode_rows([q])[0]
        assert np.array_equal(_flac_samples(tmp_path / "x.flac"), q)
