"""Characterisation of the status-word fallback ladders, on the CPU, through the public surface only.

Every ``*_checked`` call leaves a device status word; ``verified`` / ``AcousticStream._device_push`` decide what to do with it.
The five owners are built WITHOUT the library (``cls.__new__``) and driven by a scripted device: ``last_status`` answers from a list of status
words that every repeat advances, ``get_option`` / ``set_option`` work on a dict and log the writes, ``forward`` (``_call`` for the stream) logs
the repeat and returns a fresh object. Each case asserts the returned object, the exact sequence of option writes and repeats, and the counters.

The file touches nothing but public names, so it runs unchanged on the commit before the ladders were shared (audiotoken_amd/fallback.py): there
every case passes except ``test_stream_counts_a_non_finite_status_that_survives_the_repeat`` (see its docstring).
"""
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd.decoder import AcousticDecoder
from audiotoken_amd.encoder import AcousticEncoder, Wav2VecBertEncoder
from audiotoken_amd.hubert import HubertEncoder
from audiotoken_amd.streaming import AcousticStream

ENC_RANGE = ("ih_f16x2", "chain_f16x2", "res_f16x2", "rvq_f16x2", "fin_f16x2")
DEC_RANGE = ("ih_f16x2", "res_f16x2", "up_f16x2", "tail_f16x2")


class Out:
    """What a call returns: compared by identity."""

    def __init__(self, tag):
        self.tag = tag

    def __repr__(self):
        return f"Out({self.tag})"


class Device:
    """The scripted device: status word (and per-layer flag row) number k is what the k-th repeat leaves; 0 = the call before `verified`."""

    def __init__(self, statuses, options, flags=None, raise_on=None, arith=None):
        self.statuses, self.flags, self.options = list(statuses), flags, dict(options)
        self.raise_on, self.arith = raise_on, arith or {}
        self.events, self.reads, self.calls, self.outs = [], [], [], []

    def script(self, statuses, flags=None):
        """A new batch on the same handle: the options stay as the last batch left them."""
        self.statuses, self.flags = list(statuses), flags
        self.events, self.reads, self.calls, self.outs = [], [], [], []

    def last_status(self):
        assert len(self.calls) < len(self.statuses), f"repeat #{len(self.calls)} was not expected (script {self.statuses})"
        return self.statuses[len(self.calls)]

    def layer_status(self):
        return list(self.flags[len(self.calls)])

    def get_option(self, name):
        self.reads.append(name)
        return self.options[name]

    def set_option(self, name, value):
        value = self.arith[value] if isinstance(value, str) else value
        self.events.append(("set", name, value))
        self.options[name] = value

    def repeat(self, *args, **kw):
        k = len(self.calls)
        self.events.append(("repeat", k))
        self.calls.append((args, kw))
        if self.raise_on == k:
            raise RuntimeError("the repeat itself failed")
        self.outs.append(Out(k))
        return self.outs[-1]

    def install(self, owner):
        for name in ("last_status", "layer_status", "get_option", "set_option"):
            setattr(owner, name, getattr(self, name))
        return owner


def off(opts):
    return [("set", o, 0) for o in opts]


def back(opts, values=None):
    return [("set", o, (values or {}).get(o, 1)) for o in opts]


def rep(k):
    return ("repeat", k)


# ======================================================================================================
# EnCodec family: AcousticEncoder.verified, AcousticDecoder.verified, AcousticStream._device_push
# ======================================================================================================
class Acoustic:
    """One of the three owners over a scripted device. `run()` makes the public call; `counters` is the object that carries the counters."""

    def __init__(self, kind, statuses, batch=4, options=None, raise_on=None):
        self.kind, self.first = kind, Out("first")
        self.range = DEC_RANGE if kind == "decoder" else ENC_RANGE
        opts = {"lstm_pipe": 1, "persistent_lstm": 1, **{o: 1 for o in self.range}, **(options or {})}
        self.dev = dev = Device(statuses, opts, raise_on=raise_on)
        cls = AcousticDecoder if kind == "decoder" else AcousticEncoder
        self.counters = owner = cls.__new__(cls)
        torch.nn.Module.__init__(owner)
        owner.fallback_batches = 0
        if kind != "decoder":
            owner.nonfinite_batches = 0
        dev.install(owner)
        if kind == "encoder":
            self.args = (torch.zeros(batch, 8), torch.ones(batch, 8))
            owner.forward = dev.repeat
            self.run = lambda: owner.verified(self.first, *self.args)
        elif kind == "decoder":
            self.args = (torch.zeros(batch, 8, 3, dtype=torch.long),)
            owner.forward = dev.repeat
            self.run = lambda: owner.verified(self.first, *self.args)
        else:
            self.args = (torch.zeros(batch, 640), False)
            self.stream = s = AcousticStream.__new__(AcousticStream)
            s._enc, s.batch = owner, batch
            self.state = [object(), object()]
            s._state = list(self.state)
            pending = [self.first]
            s._call = lambda *a, **kw: pending.pop() if pending else dev.repeat(*a, **kw)   # the first call is the push itself, every later one a repeat
            self.run = lambda: s._device_push(*self.args)

    def check(self, events, fallback=0, nonfinite=0, swapped=True):
        assert self.dev.events == events
        assert self.counters.fallback_batches == fallback
        if self.kind != "decoder":
            assert self.counters.nonfinite_batches == nonfinite
        for args, kw in self.dev.calls:   # every repeat gets the very arguments of the first call
            assert len(args) == len(self.args) and all(a is b for a, b in zip(args, self.args)) and kw == {}
        if self.kind == "stream":   # the two state buffers change places exactly when the push succeeded
            assert self.stream._state == (self.state[::-1] if swapped else self.state)


KINDS = ("encoder", "decoder", "stream")
WITH_BIT2 = ("encoder", "stream")


@pytest.mark.parametrize("kind", KINDS)
def test_status_zero_returns_the_first_result_untouched(kind):
    a = Acoustic(kind, [0])
    assert a.run() is a.first
    a.check([])
    assert a.dev.reads == []


@pytest.mark.parametrize("kind", WITH_BIT2)
def test_non_finite_alone_is_counted_and_not_repeated(kind):
    a = Acoustic(kind, [4])
    assert a.run() is a.first
    a.check([], nonfinite=1)
    assert a.dev.reads == []


def test_decoder_knows_no_bit_two():
    """Any non-zero status of a decode is repeated, and raises when it stays."""
    a = Acoustic("decoder", [4, 0])
    assert a.run() is a.dev.outs[0]
    a.check([rep(0)])
    a = Acoustic("decoder", [4, 4])
    with pytest.raises(_cabi.HipLibraryError):
        a.run()
    a.check([rep(0)])
    a = Acoustic("decoder", [6, 4])
    with pytest.raises(_cabi.HipLibraryError):
        a.run()
    a.check(off(DEC_RANGE) + [rep(0)] + back(DEC_RANGE), fallback=1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("batch, pipe, moved", [(4, 1, "lstm_pipe"), (80, 1, "lstm_pipe"), (81, 1, "persistent_lstm"), (4, 0, "persistent_lstm")])
def test_lstm_timeout_moves_one_route_for_good(kind, batch, pipe, moved):
    a = Acoustic(kind, [1, 0], batch=batch, options={"lstm_pipe": pipe})
    assert a.run() is a.dev.outs[0]
    a.check([("set", moved, 0), rep(0)])
    assert a.dev.options[moved] == 0   # never restored


@pytest.mark.parametrize("kind", KINDS)
def test_second_lstm_timeout_takes_the_next_route(kind):
    a = Acoustic(kind, [1, 1, 0])
    assert a.run() is a.dev.outs[1]
    a.check([("set", "lstm_pipe", 0), rep(0), ("set", "persistent_lstm", 0), rep(1)])
    assert a.dev.options["lstm_pipe"] == 0 and a.dev.options["persistent_lstm"] == 0


@pytest.mark.parametrize("kind", KINDS)
def test_lstm_timeout_on_the_last_route_raises(kind):
    a = Acoustic(kind, [1, 1], batch=81)
    with pytest.raises(_cabi.HipLibraryError):
        a.run()
    a.check([("set", "persistent_lstm", 0), rep(0)], swapped=False)
    a = Acoustic(kind, [1, 1, 1])
    with pytest.raises(_cabi.HipLibraryError):
        a.run()
    a.check([("set", "lstm_pipe", 0), rep(0), ("set", "persistent_lstm", 0), rep(1)], swapped=False)


@pytest.mark.parametrize("kind", KINDS)
def test_range_overflow_repeats_that_batch_and_switches_back(kind):
    a = Acoustic(kind, [2, 0])
    assert a.run() is a.dev.outs[0]
    a.check(off(a.range) + [rep(0)] + back(a.range), fallback=1)
    assert a.dev.reads == list(a.range)


@pytest.mark.parametrize("kind", KINDS)
def test_range_option_that_was_off_stays_off(kind):
    a = Acoustic(kind, [2, 0], options={"res_f16x2": 0})
    assert a.run() is a.dev.outs[0]
    a.check(off(a.range) + [rep(0)] + back(a.range, {"res_f16x2": 0}), fallback=1)


@pytest.mark.parametrize("kind", KINDS)
def test_both_fallbacks_in_one_batch(kind):
    a = Acoustic(kind, [3, 0])
    assert a.run() is a.dev.outs[0]
    a.check([("set", "lstm_pipe", 0)] + off(a.range) + [rep(0)] + back(a.range), fallback=1)
    a = Acoustic(kind, [3, 1, 0])
    assert a.run() is a.dev.outs[1]
    a.check([("set", "lstm_pipe", 0)] + off(a.range) + [rep(0), ("set", "persistent_lstm", 0), rep(1)] + back(a.range), fallback=1)


@pytest.mark.parametrize("kind", KINDS)
def test_overflow_with_its_own_infinity_is_cured_by_the_repeat(kind):
    """Status 6: with bit 1 set the infinity descends from the fp16 overflow, so it is not counted as a non-finite input."""
    a = Acoustic(kind, [6, 0])
    assert a.run() is a.dev.outs[0]
    a.check(off(a.range) + [rep(0)] + back(a.range), fallback=1, nonfinite=0)


def test_encoder_counts_a_non_finite_status_that_survives_the_repeat():
    a = Acoustic("encoder", [6, 4])
    assert a.run() is a.dev.outs[0]
    a.check(off(ENC_RANGE) + [rep(0)] + back(ENC_RANGE), fallback=1, nonfinite=1)
    a = Acoustic("encoder", [5, 4])   # counted when it is seen, and again when the repeat did not clear it
    assert a.run() is a.dev.outs[0]
    a.check([("set", "lstm_pipe", 0), rep(0)], nonfinite=2)


def test_stream_counts_a_non_finite_status_that_survives_the_repeat():
    """The one deliberate change of the shared ladder: a push whose repeat still reports bit 2 is counted (and logged) as
    ``AcousticEncoder.verified`` counts it. Before audiotoken_amd/fallback.py the stream's own copy of the ladder left it out (it counted 0 and 1
    here), so on that commit this case, and only this one, fails."""
    a = Acoustic("stream", [6, 4])
    assert a.run() is a.dev.outs[0]
    a.check(off(ENC_RANGE) + [rep(0)] + back(ENC_RANGE), fallback=1, nonfinite=1)
    a = Acoustic("stream", [5, 4])
    assert a.run() is a.dev.outs[0]
    a.check([("set", "lstm_pipe", 0), rep(0)], nonfinite=2)


@pytest.mark.parametrize("kind", WITH_BIT2)
def test_non_finite_with_a_timeout_is_counted_and_repeated(kind):
    a = Acoustic(kind, [5, 0])
    assert a.run() is a.dev.outs[0]
    a.check([("set", "lstm_pipe", 0), rep(0)], nonfinite=1)


@pytest.mark.parametrize("kind", KINDS)
def test_a_repeat_that_raises_still_restores_the_options(kind):
    a = Acoustic(kind, [2], raise_on=0, options={"ih_f16x2": 0})
    with pytest.raises(RuntimeError, match="the repeat itself failed"):
        a.run()
    a.check(off(a.range) + [rep(0)] + back(a.range, {"ih_f16x2": 0}), fallback=1, swapped=False)


@pytest.mark.parametrize("kind", KINDS)
def test_a_status_that_stays_raises_and_restores_the_options(kind):
    a = Acoustic(kind, [2, 2])
    with pytest.raises(_cabi.HipLibraryError):
        a.run()
    a.check(off(a.range) + [rep(0)] + back(a.range), fallback=1, swapped=False)


def test_range_option_lists():
    assert AcousticEncoder.RANGE_OPTIONS == ENC_RANGE


# ======================================================================================================
# semantic family: Wav2VecBertEncoder.verified, HubertEncoder.verified
# ======================================================================================================
class Semantic:
    """semantic_m ("m") or semantic_s ("s") over a scripted device. Flag rows are written per LAYER; semantic_s' own flag 0 (front end) is `front`."""

    def __init__(self, kind, statuses, flags, options=None, raise_on=None):
        self.kind, self.first = kind, Out("first")
        cls = Wav2VecBertEncoder if kind == "m" else HubertEncoder
        self.dev = dev = Device(statuses, {"arith": 2, **(options or {})}, flags=self.rows(flags), raise_on=raise_on, arith=cls.ARITH)
        self.owner = owner = cls.__new__(cls)
        torch.nn.Module.__init__(owner)
        owner.fallback_batches = owner.nonfinite_batches = 0
        owner.pinned_layers, owner.layer_overflows = [], {}
        dev.install(owner)
        owner.forward = dev.repeat
        self.args = (torch.zeros(2, 8), torch.ones(2, 8))

    def rows(self, flags):
        out = []
        for row in flags:
            front = 0
            if isinstance(row, dict):
                front, row = row["front"], row["layers"]
            assert self.kind == "s" or front == 0
            out.append(([front] if self.kind == "s" else []) + list(row))
        return out

    def script(self, statuses, flags):
        self.dev.script(statuses, self.rows(flags))

    def run(self, **kw):
        return self.owner.verified(self.first, *self.args, **kw)

    def check(self, events, fallback=0, nonfinite=0, overflows=None, pinned=(), kw=None):
        o = self.owner
        assert self.dev.events == events
        assert (o.fallback_batches, o.nonfinite_batches) == (fallback, nonfinite)
        assert o.layer_overflows == (overflows or {}) and list(o.pinned_layers) == list(pinned)
        for args, k in self.dev.calls:
            assert len(args) == 2 and all(a is b for a, b in zip(args, self.args)) and k == (kw or {})


def layer(l, v):
    return ("set", f"layer_arith:{l}", v)


SEM = ("m", "s")


@pytest.mark.parametrize("kind", SEM)
def test_semantic_status_zero_and_non_finite_alone(kind):
    s = Semantic(kind, [0], [[0, 0]])
    assert s.run() is s.first
    s.check([])
    assert s.dev.reads == []
    s = Semantic(kind, [4], [[0, 0]])
    assert s.run() is s.first
    s.check([], nonfinite=1)
    assert s.dev.reads == []


@pytest.mark.parametrize("kind", SEM)
def test_first_overflow_of_a_layer_is_transient(kind):
    """An overflow turns into infinities that every later layer flags too: the FIRST flagged layer is moved, for this batch only."""
    s = Semantic(kind, [2, 0], [[0, 0, 2, 2], [0, 0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([layer(2, 1), rep(0), layer(2, -1)], fallback=1, overflows={2: 1})


@pytest.mark.parametrize("kind", SEM)
def test_layer_is_pinned_from_its_pin_after_th_overflowing_batch(kind):
    s = Semantic(kind, [2, 0], [[0, 0, 2, 2], [0, 0, 0, 0]])
    assert type(s.owner).PIN_AFTER == 2
    for n in range(1, type(s.owner).PIN_AFTER):
        s.script([2, 0], [[0, 0, 2, 2], [0, 0, 0, 0]])
        assert s.run() is s.dev.outs[0]
        s.check([layer(2, 1), rep(0), layer(2, -1)], fallback=n, overflows={2: n})
    n = type(s.owner).PIN_AFTER
    s.script([2, 0], [[0, 0, 2, 2], [0, 0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([layer(2, 1), rep(0)], fallback=n, overflows={2: n}, pinned=[2])     # not restored
    assert s.dev.options["layer_arith:2"] == 1
    s.script([0], [[0, 0, 0, 0]])
    s.owner.unpin_layers()
    s.check([layer(2, -1)], fallback=n)


@pytest.mark.parametrize("kind", SEM)
def test_three_layers_in_one_batch(kind):
    s = Semantic(kind, [2, 2, 2, 0], [[2, 2, 2, 2], [0, 2, 2, 2], [0, 0, 2, 2], [0, 0, 0, 0]])
    assert s.run() is s.dev.outs[2]
    s.check([layer(0, 1), rep(0), layer(1, 1), rep(1), layer(2, 1), rep(2), layer(0, -1), layer(1, -1), layer(2, -1)],
            fallback=1, overflows={0: 1, 1: 1, 2: 1})


@pytest.mark.parametrize("kind", SEM)
@pytest.mark.parametrize("arith", [2, 0])
def test_a_fourth_layer_sends_the_batch_to_the_whole_model_repeat(kind, arith):
    """... with `arith` saved, set to bf16x3 (1) and set back to what was read (0 stays 0)."""
    s = Semantic(kind, [2, 2, 2, 2, 0], [[2, 2, 2, 2], [0, 2, 2, 2], [0, 0, 2, 2], [0, 0, 0, 2], [0, 0, 0, 0]], options={"arith": arith})
    assert s.run() is s.dev.outs[3]
    s.check([layer(0, 1), rep(0), layer(1, 1), rep(1), layer(2, 1), rep(2), layer(0, -1), layer(1, -1), layer(2, -1),
             ("set", "arith", 1), rep(3), ("set", "arith", arith)], fallback=1, overflows={0: 1, 1: 1, 2: 1})


@pytest.mark.parametrize("kind", SEM)
def test_no_layer_flagged_goes_to_the_whole_model_repeat(kind):
    s = Semantic(kind, [2, 0], [[0, 0, 0], [0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([("set", "arith", 1), rep(0), ("set", "arith", 2)], fallback=1)
    assert s.dev.reads == ["arith"]


def test_semantic_s_front_end_overflow_goes_to_the_whole_model_repeat():
    """Flag 0 of semantic_s is the conv feature encoder + positional conv: a property of the input's level, no layer is moved or counted."""
    s = Semantic("s", [2, 0], [{"front": 2, "layers": [2, 2, 2]}, [0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([("set", "arith", 1), rep(0), ("set", "arith", 2)], fallback=1)


@pytest.mark.parametrize("kind", SEM)
@pytest.mark.parametrize("first", [2, 6])
def test_non_finite_after_a_layer_repeat_is_counted(kind, first):
    s = Semantic(kind, [first, 4], [[0, 2, 2], [0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([layer(1, 1), rep(0), layer(1, -1)], fallback=1, nonfinite=1, overflows={1: 1})


@pytest.mark.parametrize("kind", SEM)
def test_non_finite_after_the_whole_model_repeat_is_counted(kind):
    s = Semantic(kind, [6, 4], [[0, 0, 0], [0, 0, 0]])
    assert s.run() is s.dev.outs[0]
    s.check([("set", "arith", 1), rep(0), ("set", "arith", 2)], fallback=1, nonfinite=1)


@pytest.mark.parametrize("kind", SEM)
def test_layer_flagged_again_in_the_same_batch(kind):
    """The same layer overflowing on bf16x3 too is counted again: with PIN_AFTER = 2 that pins it, and the batch's end still sets it back once."""
    s = Semantic(kind, [2, 2, 0], [[0, 2], [0, 2], [0, 0]])
    assert s.run() is s.dev.outs[1]
    s.check([layer(1, 1), rep(0), layer(1, 1), rep(1), layer(1, -1)], fallback=1, overflows={1: 2}, pinned=[1])


@pytest.mark.parametrize("kind", SEM)
def test_semantic_status_that_stays_raises_and_restores_arith(kind):
    s = Semantic(kind, [2, 2], [[0, 0], [0, 0]], options={"arith": 0})
    with pytest.raises(_cabi.HipLibraryError):
        s.run()
    s.check([("set", "arith", 1), rep(0), ("set", "arith", 0)], fallback=1)


@pytest.mark.parametrize("kind", SEM)
def test_semantic_repeat_that_raises_restores_what_it_moved(kind):
    s = Semantic(kind, [2], [[0, 2]], raise_on=0)
    with pytest.raises(RuntimeError, match="the repeat itself failed"):
        s.run()
    s.check([layer(1, 1), rep(0), layer(1, -1)], fallback=1, overflows={1: 1})
    s = Semantic(kind, [2], [[0, 0]], raise_on=0)
    with pytest.raises(RuntimeError, match="the repeat itself failed"):
        s.run()
    s.check([("set", "arith", 1), rep(0), ("set", "arith", 2)], fallback=1)


def test_semantic_m_forwards_its_keyword_arguments_to_every_repeat():
    s = Semantic("m", [2, 2, 2, 2, 0], [[2, 2, 2, 2], [0, 2, 2, 2], [0, 0, 2, 2], [0, 0, 0, 2], [0, 0, 0, 0]])
    assert s.run(pad_to_multiple_of=4, n_layers=3) is s.dev.outs[3]
    assert len(s.dev.calls) == 4
    s.check([layer(0, 1), rep(0), layer(1, 1), rep(1), layer(2, 1), rep(2), layer(0, -1), layer(1, -1), layer(2, -1),
             ("set", "arith", 1), rep(3), ("set", "arith", 2)], fallback=1, overflows={0: 1, 1: 1, 2: 1}, kw={"pad_to_multiple_of": 4, "n_layers": 3})


def test_semantic_classes_share_their_policy_constants():
    assert Wav2VecBertEncoder.PIN_AFTER == HubertEncoder.PIN_AFTER == 2
    assert Wav2VecBertEncoder.ARITH == HubertEncoder.ARITH == {"f32": 0, "bf16x3": 1, "f16x2": 2}
