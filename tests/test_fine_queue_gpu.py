"""GPU: the fine stage's window queue (csrc/fine.hip at_fine_generate_queue, ``CoarseToFine.generate_queue``, ``AudioToken.to_fine(slots=)``; DESIGN.md
§21) against the CPU twin of tests/fine_ref.py, by §18's protocol restated for ragged draws (tests/fine_queue_cases.verify), and against ``generate`` on
each row alone: a row's result must not depend on the slot, the pass or the neighbours it ran with."""
import ctypes as C

import numpy as np
import pytest
import torch

from audiotoken_amd import _cabi
from audiotoken_amd.fine_decoder import CoarseToFine, fine_queue_passes, row_uniforms

from tests import fine_cases as K
from tests import fine_queue_cases as Q
from tests import fine_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RECORD = {"max_logit_diff": 0.0, "waived": 0, "draws": 0}
_decoders = {}


def decoder(m, family):
    if (m, family) not in _decoders:
        _decoders[(m, family)] = CoarseToFine(device=DEV, weights=K.weights(m, family))
    return _decoders[(m, family)]


def inputs(lengths, W, order=None):
    order = list(range(len(lengths))) if order is None else order
    return [Q.row(i, lengths[i]) for i in order], [Q.draws(i, lengths[i], W) for i in order]


def alone(dec, row, u, temperature=K.TEMPERATURE, return_logits=False):
    return dec.generate(row, temperature=temperature, uniforms=None if temperature is None else u[None], return_logits=return_logits)


def record(worst, waived, draws):
    RECORD["max_logit_diff"] = max(RECORD["max_logit_diff"], worst)
    RECORD["waived"] += waived
    RECORD["draws"] += draws
    print(f"so far: largest logit difference {RECORD['max_logit_diff']:.3e}; waived {RECORD['waived']} of {RECORD['draws']} draws")


def check_schedule(gen, lengths, W, slots):
    passes, placement = fine_queue_passes(lengths, W, slots)
    assert gen.placement == placement, "the library's placement equals the twin's"
    assert len(gen.passes) == len(passes)
    for p, (got, want) in enumerate(zip(gen.passes, passes)):
        admitted = sum(1 for _, _, k in want if k == 0)
        retired = sum(1 for b in range(len(lengths)) if placement[b][2] == p)
        assert got == (len(want), admitted, retired), f"pass {p}"
    return passes


@pytest.mark.parametrize("m", ["a", "b"])
@pytest.mark.parametrize("order", ["forwards", "reversed"])
def test_one_slot_equals_each_row_alone_bit_for_bit(m, order):
    """slots = 1: a pass is one window, so a row's launches are those of ``generate`` on the row alone: codes AND logits are bit-equal. Reversed, every
    row but the first enters a slot that a longer row has just left: no stale cell may be read."""
    W = K.MODELS[m]["block"]
    lengths = Q.single_slot_lengths(W)
    idx = list(range(len(lengths)))[::-1 if order == "reversed" else 1]
    dec = decoder(m, "peaky")
    rows, u = inputs(lengths, W, idx)
    gen = dec.generate_queue(rows, slots=1, temperature=K.TEMPERATURE, uniforms=u, return_logits=True)
    check_schedule(gen, [lengths[i] for i in idx], W, 1)
    assert all(p[0] == 1 for p in gen.passes) and len(gen.passes) == sum(len(R.fine_windows(T, W)) for T in lengths)
    for j, i in enumerate(idx):
        one = alone(dec, rows[j], u[j], return_logits=True)
        assert torch.equal(gen.codes[j], one.codes[0]), f"row of {lengths[i]} frames: other codes than alone"
        assert torch.equal(gen.window_ids[j], one.window_ids[0])
        assert torch.equal(torch.nan_to_num(gen.logits[j], nan=-7.0), torch.nan_to_num(one.logits[0], nan=-7.0)), f"row of {lengths[i]} frames: other logits than alone"


@pytest.mark.parametrize("family", K.FAMILIES)
@pytest.mark.parametrize("m", ["a", "b"])
def test_mixed_passes_meet_the_protocol_and_equal_each_row_alone(m, family):
    W = K.MODELS[m]["block"]
    lengths = Q.mixed_lengths(W)
    assert [len(R.fine_windows(T, W)) for T in lengths] == Q.MIXED_WINDOWS
    w, dec = K.weights(m, family), decoder(m, family)
    rows, u = inputs(lengths, W)
    gen = dec.generate_queue(rows, slots=4, temperature=K.TEMPERATURE, uniforms=u, return_logits=True)
    record(*Q.verify(w, W, rows, gen, u, K.TEMPERATURE, raw=dec.last_raw_codes))
    passes = check_schedule(gen, lengths, W, 4)
    assert any(len({k for _, _, k in p}) > 1 for p in passes), "at least one pass holds windows of different k"
    assert any(got[0] > 1 and got[1] > 0 and got[1] < got[0] for got in gen.passes), "the device's trace shows a pass that admits next to running rows"
    singles = [alone(dec, rows[b], u[b]).codes[0] for b in range(len(rows))]
    for b in range(len(rows)):
        assert torch.equal(gen.codes[b], singles[b]), f"row {b} alone, with its own draws, gives other codes than in the queue"
    # reversed: other slots, other passes, other neighbours; every row keeps its codes
    idx = list(range(len(lengths)))[::-1]
    rrows, ru = inputs(lengths, W, idx)
    rev = dec.generate_queue(rrows, slots=4, temperature=K.TEMPERATURE, uniforms=ru)
    rpasses = check_schedule(rev, [lengths[i] for i in idx], W, 4)
    assert any(len({k for _, _, k in p}) > 1 for p in rpasses)
    assert rev.placement != [gen.placement[i] for i in idx], "the reversed order places rows elsewhere"
    for j, i in enumerate(idx):
        assert torch.equal(rev.codes[j], singles[i]), f"row {i} in the reversed queue gives other codes than alone"


def test_more_rows_than_slots_twice_in_one_state():
    W = K.MODELS["a"]["block"]
    lengths = [W // 2] * 130
    dec = decoder("a", "peaky")
    rows, u = inputs(lengths, W)
    first = dec.generate_queue(rows, slots=64, temperature=K.TEMPERATURE, uniforms=u)
    state = dec._ws.data_ptr()
    second = dec.generate_queue(rows, slots=64, temperature=K.TEMPERATURE, uniforms=u)
    assert dec._ws.data_ptr() == state, "the second run used the first one's state"
    assert first.passes == [(64, 64, 64), (64, 64, 64), (2, 2, 2)] == second.passes
    assert all(torch.equal(p, q) for p, q in zip(first.codes, second.codes))
    assert len({tuple(c[2].tolist()) for c in first.codes}) == 130, "rows with different inputs and draws"
    for b in (0, 63, 64, 129):   # the first and last row of a slot's first tenure, and rows that entered a used slot
        assert torch.equal(first.codes[b], alone(dec, rows[b], u[b]).codes[0])


@pytest.mark.parametrize("m", ["a", "b"])
def test_argmax_path_on_a_mixed_pass_has_no_waiver(m):
    W = K.MODELS[m]["block"]
    lengths = [W + W // 2 + 1, 7, W + 1, W]
    w, dec = K.weights(m, "peaky"), decoder(m, "peaky")
    rows, _ = inputs(lengths, W)
    gen = dec.generate_queue(rows, slots=2, temperature=None, return_logits=True)
    passes = check_schedule(gen, lengths, W, 2)
    assert any(len({k for _, _, k in p}) > 1 for p in passes)
    worst, waived, draws = Q.verify(w, W, rows, gen, None, None, raw=dec.last_raw_codes)
    assert waived == 0
    for b, r in enumerate(rows):
        assert torch.equal(gen.codes[b], alone(dec, r, None, temperature=None).codes[0])


def test_a_code_outside_its_range_raises():
    dec = decoder("a", "uniform")
    good = [K.coarse_row(10), K.coarse_row(200)]
    for value in (1024, -1):
        bad = K.coarse_row(150)
        bad[1, 140] = value
        with pytest.raises(ValueError, match="outside"):
            dec.generate_queue(good + [bad], slots=2)
    assert [c.shape for c in dec.generate_queue(good, slots=2, temperature=None).codes] == [(8, 10), (8, 200)], "the handle goes on working"


def test_refusals_touch_nothing():
    """Every refusal comes before any launch: the status word and the output keep the values put there."""
    dec = decoder("a", "uniform")
    W = dec.block_size
    rows = [K.coarse_row(10), K.coarse_row(200)]
    with pytest.raises(ValueError, match="slots"):
        dec.generate_queue(rows, slots=0)
    with pytest.raises(ValueError, match="slots"):
        dec.generate_queue(rows, slots=65)
    with pytest.raises(ValueError, match="rows"):
        dec.generate_queue([], slots=4)
    with pytest.raises(ValueError, match="rows"):
        dec.generate_queue([K.coarse_row(1)] * 4097, slots=4)
    with pytest.raises(ValueError, match=r"\[2, T\]"):
        dec.generate_queue([K.coarse_row(10), np.zeros((2, 0), dtype=np.int64)], slots=4)
    assert [len(R.fine_windows(r.shape[1], W)) for r in rows] == [1, 3]
    for u in ([row_uniforms(0, 0, 1, W)], [row_uniforms(0, 0, 1, W), row_uniforms(0, 1, 2, W)], [row_uniforms(0, 0, 1, W), row_uniforms(0, 1, 3, W)[:, :5]],
              np.zeros((2, 2, 6, W), dtype=np.float32)):
        with pytest.raises(ValueError, match="uniforms"):
            dec.generate_queue(rows, slots=4, uniforms=u)
    # the library itself, on device buffers that hold sentinels
    lib = _cabi.load()
    lens = [10, 200]
    n = sum(len(R.fine_windows(T, W)) for T in lens)
    coarse = torch.zeros(2 * sum(lens), dtype=torch.int32, device=DEV)
    out = torch.full((8 * sum(lens),), -5, dtype=torch.int32, device=DEV)
    status = torch.full((1,), 77, dtype=torch.int32, device=DEV)
    u = torch.zeros(n * 6 * W, dtype=torch.float32, device=DEV)
    need = int(lib.at_fine_queue_state_bytes(dec.handle, 4, 200))
    assert need > 0 and need == int(lib.at_fine_state_bytes(dec.handle, 4, 200))
    state = torch.zeros(need, dtype=torch.uint8, device=DEV)
    stream = _cabi.current_stream_handle(torch.device(DEV))

    def call(lens=lens, n_rows=2, slots=4, state_bytes=need, max_T=200):
        c_lens = (C.c_int32 * max(len(lens), 1))(*lens)
        passes = (C.c_int32 * 1)(-3)
        rc = lib.at_fine_generate_queue(dec.handle, coarse.data_ptr(), c_lens, n_rows, 0.5, 0, u.data_ptr(), out.data_ptr(), None, None, state.data_ptr(),
                                        state_bytes, max_T, slots, None, 0, passes, None, stream, status.data_ptr())
        return rc, passes[0], _cabi.last_error()

    for kw, text in ((dict(slots=0), "slots"), (dict(slots=65), "slots"), (dict(n_rows=0), "n_rows"), (dict(n_rows=4097), "n_rows"),
                     (dict(lens=[10, 0]), "row 1"), (dict(max_T=199), "row 1"), (dict(state_bytes=need - 1), "state too small")):
        rc, passes, err = call(**kw)
        assert rc != 0 and passes == -3 and text in err, (kw, err)
    torch.cuda.synchronize()
    assert int(status.item()) == 77 and bool((out == -5).all()), "a refused call touches neither the status nor the output"
    rc, passes, err = call()
    assert rc == 0 and passes == 3, err     # the row of 200 frames has three windows
    torch.cuda.synchronize()
    assert bool((out >= 0).all()) and int(status.item()) == 77


def test_to_fine_slots_from_seed_equals_the_documented_draws():
    from audiotoken_amd import AudioToken
    from audiotoken_amd.configs import Tokenizers
    at = AudioToken(Tokenizers.acoustic, device=DEV, fine_weights=K.weights("a", "uniform"))
    lengths = [70, 200, 129]
    rows = [K.coarse_row(T) for T in lengths]
    a = at.to_fine(rows, temperature=1.0, seed=3, slots=2)
    by_rule = [np.random.Generator(np.random.Philox(key=[3, b])).random((len(R.fine_windows(T, 128)), 6, 128), dtype=np.float32) for b, T in enumerate(lengths)]
    b = at.to_fine(rows, temperature=1.0, uniforms=by_rule, slots=2)
    c = at.to_fine(rows, temperature=1.0, seed=4, slots=2)
    assert a.passes == b.passes and a.placement == [(0, 0, 0), (1, 0, 2), (0, 1, 2)]
    assert all(torch.equal(p, q) for p, q in zip(a.codes, b.codes))
    assert not all(torch.equal(p, q) for p, q in zip(a.codes, c.codes)), "another seed gives other draws"
    # a row's draws from the seed do not depend on the other rows' lengths: row 1 keeps its codes next to other neighbours
    d = at.to_fine([K.coarse_row(300), rows[1]], temperature=1.0, seed=3, slots=1)
    assert torch.equal(d.codes[1], a.codes[1])
    with pytest.raises(ValueError, match="64"):
        at.to_fine([K.coarse_row(1)] * 65)
    assert at.to_fine(rows[:2], temperature=None).passes is None, "without slots= nothing changes"
