"""audiotoken_amd/fallback.py driven directly: the owner is a plain object, so the policy needs neither a torch module nor the library.
(tests/test_fallback_cpu.py pins the same ladders through the five public owners.)"""
import pytest

from audiotoken_amd import _cabi, fallback

RANGE = ("a_f16x2", "b_f16x2")


class Owner:
    PIN_AFTER = 2

    def __init__(self, statuses, flags=None, **options):
        self.statuses, self.flags = statuses, flags
        self.options = {"lstm_pipe": 1, "persistent_lstm": 1, "a_f16x2": 1, "b_f16x2": 0, "arith": 2, **options}
        self.events, self.repeats = [], 0
        self.fallback_batches = self.nonfinite_batches = 0
        self.pinned_layers, self.layer_overflows = [], {}

    def last_status(self):
        return self.statuses[self.repeats]

    def layer_status(self):
        return self.flags[self.repeats]

    def get_option(self, name):
        return self.options[name]

    def set_option(self, name, value):
        self.events.append((name, value))
        self.options[name] = value

    def rerun(self):
        self.repeats += 1
        self.events.append(("repeat", self.repeats))
        return f"repeat {self.repeats}"


def encodec(o, batch=4, **kw):
    return fallback.encodec_ladder(o, "first", o.rerun, batch, RANGE, "test call", **kw)


def semantic(o, first_layer_flag=0):
    return fallback.semantic_ladder(o, "first", o.rerun, first_layer_flag, "test", "test call")


def test_encodec_ladder_on_a_plain_object():
    o = Owner([0])
    assert encodec(o) == "first" and o.events == []
    o = Owner([4])
    assert encodec(o) == "first" and o.events == [] and o.nonfinite_batches == 1
    o = Owner([3, 1, 4])
    assert encodec(o) == "repeat 2"
    assert o.events == [("lstm_pipe", 0), ("a_f16x2", 0), ("b_f16x2", 0), ("repeat", 1), ("persistent_lstm", 0), ("repeat", 2), ("a_f16x2", 1), ("b_f16x2", 0)]
    assert (o.fallback_batches, o.nonfinite_batches) == (1, 1)
    o = Owner([1, 0])
    assert encodec(o, batch=81) == "repeat 1" and o.events == [("persistent_lstm", 0), ("repeat", 1)]


def test_encodec_ladder_without_a_quantiser_raises_on_any_status_left():
    o = Owner([2, 4])
    with pytest.raises(_cabi.HipLibraryError):
        encodec(o, nonfinite_bit=False)
    assert o.events == [("a_f16x2", 0), ("b_f16x2", 0), ("repeat", 1), ("a_f16x2", 1), ("b_f16x2", 0)]
    assert o.nonfinite_batches == 0


def test_semantic_ladder_on_a_plain_object():
    o = Owner([2, 0], flags=[[0, 2, 2], [0, 0, 0]])
    assert semantic(o) == "repeat 1"
    assert o.events == [("layer_arith:1", 1), ("repeat", 1), ("layer_arith:1", -1)] and o.layer_overflows == {1: 1} and o.pinned_layers == []
    o = Owner([2, 0], flags=[[0, 2, 2], [0, 0, 0]])
    assert semantic(o, first_layer_flag=1) == "repeat 1"   # the same row read as [front end, layer 0, layer 1]
    assert o.events == [("layer_arith:0", 1), ("repeat", 1), ("layer_arith:0", -1)] and o.layer_overflows == {0: 1}
    o = Owner([2, 4], flags=[[2, 2, 2], [0, 0, 0]])
    assert semantic(o, first_layer_flag=1) == "repeat 1"   # the front end: whole-model repeat, bit 2 left over is counted
    assert o.events == [("arith", "bf16x3"), ("repeat", 1), ("arith", 2)] and o.layer_overflows == {}
    assert (o.fallback_batches, o.nonfinite_batches) == (1, 1)


def test_the_decoder_publishes_its_range_options():
    from audiotoken_amd.decoder import AcousticDecoder
    assert AcousticDecoder.RANGE_OPTIONS == ("ih_f16x2", "res_f16x2", "up_f16x2", "tail_f16x2")
