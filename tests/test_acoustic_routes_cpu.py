"""CPU: the acoustic route table (tests/acoustic_routes.py) covers every length-selected kernel route, the oracle encodes every entry, and
the inputs are chosen so that the parity bar has (almost) nothing it could excuse."""
import collections

import pytest
import torch

from audiotoken_amd import weights as W
from oracle import encodec_ref as R
from tests import acoustic_routes as AR
from tests import parity as P

ALL_SIGNATURES = {(a, b, c, d, e) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1) for e in (0, 1)}


def test_signature_follows_the_length_chain():
    assert AR.chain(24000) == [24000, 12000, 3000, 600, 75]
    assert AR.chain(321) == [321, 161, 41, 9, 2]
    assert AR.signature(24000) == (1, 1, 1, 1, 1)
    assert AR.signature(12345) == (0, 0, 0, 0, 1) and AR.signature(27527) == (0, 1, 0, 0, 1)
    assert AR.signature(9999) == (0, 1, 1, 0, 1) and AR.signature(3400) == (1, 1, 1, 0, 1)
    assert AR.chain(AR.MIN_SAMPLES - 1)[3] == 8 and AR.chain(AR.MIN_SAMPLES)[3] == 9      # the library refuses L[3] <= 8


def test_table_covers_every_route():
    assert len(set(AR.LENGTHS)) == len(AR.LENGTHS)
    assert all(n >= AR.MIN_SAMPLES for n in AR.LENGTHS)
    assert {AR.signature(n) for n in AR.LENGTHS} == ALL_SIGNATURES
    # the small set: the smallest N of each signature, by exhaustive search
    first = {}
    for n in range(AR.MIN_SAMPLES, 4000):
        first.setdefault(AR.signature(n), n)
    assert sorted(first.values()) == list(AR.SMALL) and len(first) == 32
    # the mid set: every signature with e = 1 once, each with a ragged last tile in a fused kernel
    assert sorted(AR.signature(n) for n in AR.MID) == sorted(s for s in ALL_SIGNATURES if s[4] == 1)
    for n in AR.MID:
        L = AR.chain(n)
        assert 9000 <= n <= 30000
        assert L[1] % 64 != 0 and L[2] % 32 != 0, (n, L)
        if AR.signature(n)[1:4] != (1, 1, 1):      # b, c and d together leave L[1] = 160 k: no 1-row or 63-row tail exists
            assert L[1] % 64 in (1, 63) or L[2] % 32 in (1, 31), (n, L)
    # the seams: T = 256 / 257 around the 256-row pad of the GEMM operands, even and odd
    assert sorted(AR.chain(n)[4] for n in AR.SEAMS) == [256, 256, 257, 257]
    assert sorted(n % 2 for n in AR.SEAMS) == [0, 0, 1, 1]
    # the batch-side cross: an all-false signature, the stand-alone split route, a T <= 6 length
    sigs = [AR.signature(n) for n in AR.BATCH_CROSS]
    assert all(n in AR.LENGTHS for n in AR.BATCH_CROSS)
    assert sigs[0] == (0, 0, 0, 0, 0) and sigs[1][2:4] == (0, 1) and sigs[2][4] == 0


def test_expected_evidence_separates_the_routes():
    """Profile launch counts + range sites (what the GPU test reads back) tell all 32 signatures apart."""
    seen = collections.defaultdict(set)
    for s in ALL_SIGNATURES:
        launches, sites = AR.expected_launches(s), AR.expected_range_sites(s)
        key = tuple(sorted(launches.items())) + tuple(sorted((k, v) for k, v in sites.items() if k != "down2"))
        seen[key].add(s)
    assert all(len(v) == 1 for v in seen.values()), [v for v in seen.values() if len(v) > 1]


@pytest.mark.parametrize("family", AR.FAMILIES)
def test_oracle_encodes_the_table_and_has_few_near_ties(family):
    """The bar "equal, or explained by an oracle top-2 margin < RVQ_TIE" can only excuse frames on which the oracle itself has such a margin
    (at any stage). Their share over the whole table is capped at 1 %, so the bar cannot hide a route. Measured with these seeds: see the print."""
    w = W.synth_encodec_weights(seed=0, with_decoder=False, family=family)
    frames = near = 0
    smallest = float("inf")
    for n in AR.LENGTHS:
        wav = torch.from_numpy(AR.waveform(n))
        codes, margins = R.acoustic_encode(w, wav, AR.N_Q, return_margins=True)
        T = AR.chain(n)[4]
        assert tuple(codes.shape) == (AR.B, AR.N_Q, T) and codes.dtype == torch.int16
        assert torch.isfinite(margins).all()
        frames += AR.B * T
        near += int((margins.min(dim=1).values < P.RVQ_TIE).sum())
        smallest = min(smallest, float(margins.min()))
    print(f"{family}: {near} of {frames} oracle frames have a top-2 margin < {P.RVQ_TIE:g} at some stage (smallest margin {smallest:.2e})")
    assert near <= 0.01 * frames, f"{family}: {near} of {frames} frames are oracle near-ties: change the waveform seeds, not the cap"
