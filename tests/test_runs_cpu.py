"""CPU: the run log every whole-file driver writes through (audiotoken_amd/runs.py: who was skipped, the timing keys, the final report, the guard around
end-of-run bookkeeping), and the one hold step the chunked and the streamed decode loops share (audiotoken_amd/decode_files.py: ``DecodeRun.hold``), which
must drop a file at the number of held bytes each loop dropped it at when it had its own copy."""
import logging
import os

import numpy as np
import pytest

from audiotoken_amd import runs
from tests.test_stream_files_cpu import HOP, _StubDecoder, _tok, _tokens


class _Tok:
    def __init__(self):
        self.skipped_files = []


def test_skipped_appends_and_logs(caplog):
    tok = _Tok()
    log = runs.RunLog(tok, "encode_batch_files")
    with caplog.at_level(logging.ERROR):
        log.skipped("/data/a.wav", "Audio needs to be mono")
        log.skipped("/data/b.tar:x.mp3", "no decoder")
    assert tok.skipped_files == [("/data/a.wav", "Audio needs to be mono"), ("/data/b.tar:x.mp3", "no decoder")]
    assert [r.getMessage() for r in caplog.records] == ["Skipping /data/a.wav: Audio needs to be mono", "Skipping /data/b.tar:x.mp3: no decoder"]


@pytest.mark.parametrize("what,product", [("encode_batch_files", "token"), ("decode_batch_files", "audio")])
def test_report_text_for_one_and_for_nine_skipped_inputs(caplog, what, product):
    tok = _Tok()
    log = runs.RunLog(tok, what, product)
    with caplog.at_level(logging.ERROR):
        log.report()
    assert not caplog.records                     # nothing skipped: nothing to say
    tok.skipped_files.append(("f0.wav", "why 0"))
    with caplog.at_level(logging.ERROR):
        log.report()
    assert caplog.records[-1].getMessage() == f"{what}: 1 input(s) were skipped and have NO {product} file (AudioToken.skipped_files): f0.wav (why 0)"
    tok.skipped_files += [(f"f{i}.wav", f"why {i}") for i in range(1, 9)]
    with caplog.at_level(logging.ERROR):
        log.report()
    first8 = "; ".join(f"f{i}.wav (why {i})" for i in range(8))
    assert caplog.records[-1].getMessage() == f"{what}: 9 input(s) were skipped and have NO {product} file (AudioToken.skipped_files): {first8} ..."
    tok.skipped_files.pop()                       # exactly 8: all of them, no ellipsis
    with caplog.at_level(logging.ERROR):
        log.report()
    assert caplog.records[-1].getMessage().endswith("f7.wav (why 7)")


def test_timing_keys_laps_and_counters():
    log = runs.RunLog(_Tok(), "encode_batch_files")
    assert log.timings == {"stage_s": 0.0, "encode_call_s": 0.0, "device_wait_s": 0.0, "save_s": 0.0, "batches": 0, "rows": 0}
    assert list(log.timings) == ["stage_s", "encode_call_s", "device_wait_s", "save_s", "batches", "rows"]
    log.laps(("encode_call_s", "save_s", "stage_s", "device_wait_s"), 10.0, 10.5, 12.5, 12.75, 20.75)
    log.laps(("save_s",), 1.0, 1.25)
    assert (log.timings["encode_call_s"], log.timings["save_s"], log.timings["stage_s"], log.timings["device_wait_s"]) == (0.5, 2.25, 0.25, 8.0)
    log.lap("stage_s", 0.0)                       # since a perf_counter reading of 0: some positive time
    assert log.timings["stage_s"] > 0.25
    log.batch(3)
    log.batch(2)
    assert (log.timings["batches"], log.timings["rows"]) == (2, 5) and "total_s" not in log.timings
    log.finish()
    assert list(log.timings)[-1] == "total_s" and log.timings["total_s"] >= 0.0


def test_guard_swallows_a_bookkeeping_error_but_not_the_runs_own(caplog):
    log = runs.RunLog(_Tok(), "encode_batch_files")
    with caplog.at_level(logging.ERROR):
        with log.guard("end-of-run bookkeeping failed"):
            raise KeyError("pinned_layers")
    assert [r.getMessage() for r in caplog.records] == ["encode_batch_files: end-of-run bookkeeping failed: KeyError: 'pinned_layers'"]
    caplog.clear()
    with caplog.at_level(logging.ERROR), pytest.raises(RuntimeError, match="device lost"):
        try:
            raise RuntimeError("device lost")     # what ended the run ...
        finally:
            with log.guard("end-of-run bookkeeping failed"):
                raise ValueError("and the bookkeeping failed as well")      # ... is what the caller sees
    assert len(caplog.records) == 1 and "ValueError: and the bookkeeping failed as well" in caplog.records[0].getMessage()
    with log.guard("end-of-run bookkeeping failed"):
        pass                                      # nothing raised: nothing logged
    assert len(caplog.records) == 1
    with pytest.raises(KeyboardInterrupt):        # an interrupt is not a bookkeeping error
        with log.guard("end-of-run bookkeeping failed"):
            raise KeyboardInterrupt


# The smallest ``max_held_bytes`` at which a.npy (75 + 75 + 75 + 10 frames, rescale=True) is still written, found by bisection on the commit before the two
# loops shared their hold step: the chunked loop charges every row of a batch 4 * 320 * t_max bytes (4 rows x 96 000, the 10-frame row too), the streamed loop
# the samples a tick emitted (4 * 320 * 235).
@pytest.mark.parametrize("batch_size", (2, 3))
@pytest.mark.parametrize("stream,keeps_at", [(False, 384000), (True, 300800)], ids=("chunked", "streamed"))
def test_both_decode_loops_drop_a_file_at_the_threshold_they_always_had(tmp_path, stream, keeps_at, batch_size):
    assert keeps_at == (4 * 4 * HOP * 75 if not stream else 4 * HOP * (3 * 75 + 10))
    src = tmp_path / "tokens"
    src.mkdir()
    np.save(src / "a.npy", _tokens(8, 3 * 75 + 10, 1))
    np.save(src / "b.npy", _tokens(8, 75, 2))
    for limit, dropped, written in ((keeps_at - 1, ["a.npy"], ["b.wav"]), (keeps_at, [], ["a.wav", "b.wav"])):
        tok = _tok(decoder=_StubDecoder())
        out = tmp_path / f"audio{limit}"
        tok.decode_batch_files(batch_size=batch_size, outdir=out, chunk_size=1, num_workers=0, token_dir=src, rescale=True, device_writer=False,
                               stream=stream, max_held_bytes=limit)
        assert [os.path.basename(p) for p, _ in tok.skipped_files] == dropped, (limit, tok.skipped_files)
        assert sorted(os.listdir(out)) == written
        assert all("max_held_bytes" in why for _, why in tok.skipped_files)
