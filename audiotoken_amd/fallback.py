"""What the host does with the device status word of a ``*_checked`` call — the one place this policy lives.

bit 0 = a bounded wait of the persistent LSTM gave up (a property of the MACHINE: the route is switched for the life of the handle);
bit 1 = an activation exceeded the fp16 range of an f16x2 kernel (a property of THIS BATCH: it is repeated on the safe arithmetic, which is
switched back afterwards); bit 2 = a NaN / infinity reached a quantiser (counted and logged: no kernel choice changes that).

Both ladders are written against a duck-typed ``owner`` — ``last_status()``, ``get_option(name)``, ``set_option(name, value)``, the counters
``fallback_batches`` / ``nonfinite_batches`` as attributes, for the semantic ladder also ``layer_status()``, ``PIN_AFTER``, ``pinned_layers`` and
``layer_overflows`` — and a ``rerun()`` that repeats the call and returns its result. Nothing here loads the library or needs a device
(tests/test_fallback_cpu.py drives the ladders with stubs).
"""
from __future__ import annotations

from typing import Callable, Sequence

from ._cabi import HipLibraryError
from .logger import get_logger

logger = get_logger(__name__)


def _count_nonfinite(owner, what: str, where: str) -> None:
    # a non-finite sample in the waveform, as a rule. The reference emits arbitrary ids for such input without a diagnostic; here it is at least logged
    # and counted. The ids are returned as they are.
    owner.nonfinite_batches += 1
    logger.error(f"{what}: a NaN or an infinity reached the quantiser {where}; check the input waveform. "
                 f"The token ids of this batch are meaningless (non-finite batch #{owner.nonfinite_batches})")


def encodec_ladder(owner, first, rerun: Callable, batch: int, range_options: Sequence[str], what: str, nonfinite_bit: bool = True):
    """EnCodec family (``AcousticEncoder.verified``, ``AcousticDecoder.verified``, the lockstep streams and the pools of streaming.py per push). ``first`` is what the call whose
    status is being read returned; it comes back as it is when the status is 0. ``batch`` = clips in the call, ``range_options`` = the f16x2
    switches turned off for the repeat, ``what`` = noun of the log lines, ``nonfinite_bit`` = whether the call has a quantiser (bit 2)."""
    status = owner.last_status()
    if status == 0:
        return first
    if nonfinite_bit and status & 4 and not status & 2:   # (with bit 1 set the infinity descends from the flagged fp16 overflow: the repeat below cures it)
        _count_nonfinite(owner, what, f"(status {status})")
        if status & ~4 == 0:
            return first
    if status & 1:
        # the pipelined two-layer launch (lstm_pipe.hip) needs 48 co-resident workgroups per 16 clips, the layer-by-layer one 16: try that first
        option, route = (("lstm_pipe", "the layer-by-layer persistent LSTM") if owner.get_option("lstm_pipe") == 1 and batch <= 80
                         else ("persistent_lstm", "per-step LSTM launches"))
        logger.error(f"{what}: persistent LSTM hand-off timed out (status {status}): the result of this batch was discarded; "
                     f"repeating it with {route} (option {option}=0) from now on")
        owner.set_option(option, 0)
    saved = {}
    if status & 2:
        owner.fallback_batches += 1
        logger.error(f"{what}: an activation exceeded the fp16 range of the f16x2 kernels (status {status}): the result of this batch was discarded; "
                     f"repeating THIS batch without them (options {', '.join(range_options)} = 0; fallback batch #{owner.fallback_batches})")
        for opt in range_options:
            saved[opt] = owner.get_option(opt)
            owner.set_option(opt, 0)
    try:
        out = rerun()
        if owner.last_status() & 1 and owner.get_option("persistent_lstm") == 1:   # the layer-by-layer persistent launch timed out as well
            logger.error(f"{what}: persistent LSTM hand-off timed out again: repeating with per-step LSTM launches (option persistent_lstm=0) from now on")
            owner.set_option("persistent_lstm", 0)
            out = rerun()
        status = owner.last_status()
        if nonfinite_bit and status & 4:   # still non-finite on the safe kernels: it came with the input, not from the fp16 range
            _count_nonfinite(owner, what, "on the fallback kernels too")
            status &= ~4                   # (not something a repeat can clear)
        if status != 0:
            raise HipLibraryError(f"{what} failed twice (status non-zero on the fallback kernels)")
    finally:
        for opt, v in saved.items():
            owner.set_option(opt, v)
    return out


def semantic_ladder(owner, first, rerun: Callable, first_layer_flag: int, layer_noun: str, what: str):
    """Semantic family (``Wav2VecBertEncoder.verified``, ``HubertEncoder.verified``). ``first_layer_flag`` = index of layer 0 in
    ``owner.layer_status()`` (flags before it belong to the front end: an overflow there is a property of the input's level and sends the batch
    straight to the whole-model repeat), ``layer_noun`` / ``what`` = nouns of the log lines.

    Range fallback policy: a layer's FIRST overflowing batch is repeated with that layer on bf16x3 and the layer goes back to f16x2 (the outlier may
    have come with the input: one loud or clipped file must not slow down — or change the rounding of — the rest of a run); from its PIN_AFTER-th
    overflowing batch on the layer stays on bf16x3 (an activation outlier that is a property of the checkpoint would repeat every batch otherwise)."""
    status = owner.last_status()
    if status == 0:
        return first
    if status & 4 and not status & 2:   # (with bit 1 set the infinity descends from the flagged fp16 overflow: the repeat below cures it)
        _count_nonfinite(owner, what, f"(status {status})")
        if status & ~4 == 0:
            return first
    owner.fallback_batches += 1
    # Which layer? Every layer has its own row of range flags; an overflow turns into infinities that all later layers flag too, so the FIRST flagged
    # part is the cause. That layer alone is moved to bf16x3 (full fp32 exponent range); the other layers keep f16x2, so a model with one such layer pays
    # ~1 / n_layers of the bf16x3 price instead of a repeat of every batch. Up to three layers are found this way per batch; beyond that the whole batch
    # is repeated on bf16x3.
    transient = []    # layers moved for THIS batch only (their first overflow): restored below
    try:
        for _ in range(3):
            bad = [i for i, f in enumerate(owner.layer_status()) if f & 2]
            if not bad or bad[0] < first_layer_flag:
                break
            layer = bad[0] - first_layer_flag
            owner.layer_overflows[layer] = owner.layer_overflows.get(layer, 0) + 1
            pin = owner.layer_overflows[layer] >= owner.PIN_AFTER
            (owner.pinned_layers if pin else transient).append(layer)
            logger.error(f"{what} reported status {status}: an activation of {layer_noun} layer {layer} exceeded the fp16 range of the f16x2 arithmetic "
                         f"(batch #{owner.layer_overflows[layer]} on which it did). The tokens of this batch were discarded; layer {layer} runs on bf16x3 "
                         f"(option layer_arith:{layer} = 1) " + ("from now on" if pin else "for this batch") +
                         f", this batch is re-encoded (fallback batch #{owner.fallback_batches})")
            owner.set_option(f"layer_arith:{layer}", 1)
            out = rerun()
            status = owner.last_status()
            if not status & 2:
                if status & 4:
                    _count_nonfinite(owner, what, f"with layer {layer} on bf16x3 too")
                return out
    finally:
        for layer in transient:
            owner.set_option(f"layer_arith:{layer}", -1)
    logger.error(f"{what} reports status {status}: the tokens of this batch were discarded; re-encoding THIS batch with arith=bf16x3 for the whole model "
                 f"(fallback batch #{owner.fallback_batches})")
    saved = owner.get_option("arith")
    owner.set_option("arith", "bf16x3")
    try:
        out = rerun()
        status = owner.last_status()
        if status & 4:          # still non-finite on the safe kernels: it came with the input, not from the fp16 range
            _count_nonfinite(owner, what, "on the fallback kernels too")
        if status & ~4 != 0:    # (bit 2, non-finite input, is not something a repeat can clear)
            raise HipLibraryError(f"{what} failed twice (status non-zero with bf16x3 arithmetic)")
    finally:
        owner.set_option("arith", saved)
    return out
