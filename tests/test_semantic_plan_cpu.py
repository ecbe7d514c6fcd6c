"""The semantic workspace plans, pinned: the size and token-count functions of the two semantic tokenizers' C ABI (pure host code, NULL handle, no
device) against a table recorded before the encode bodies of w2vbert.hip and hubert.hip were split into stages. A plan is what a caller allocates
from, so a refactor of the host code must leave every figure as it was; the table is a literal so that the test passes on both sides of that change.

semantic_m: the shortest clip (560 samples = two frames) and one sample less, T = 2, 32 / 33 (around a pad multiple of 4), 150 and 1749 tokens, each
with pad multiple 0 and 4. semantic_s: the shortest clip (400 samples) and one sample less, T = 3, 33, 256 (a full row tile) and 299. B = 1, 3, 64
and 300 for both.
"""
from audiotoken_amd import _cabi

BATCHES = (1, 3, 64, 300)
M_LENGTHS = (559, 560, 880, 10480, 10800, 48400, 560000)
M_PADS = (0, 4)
S_LENGTHS = (399, 400, 1200, 10640, 82000, 96077)


def measure(lib):
    """{name: figures}, in the order of the module constants: [length][pad][batch] for semantic_m, [length][batch] for semantic_s."""
    return {
        "semantic_m_workspace": [[[lib.at_w2vbert_workspace_bytes(None, b, n, m) for b in BATCHES] for m in M_PADS] for n in M_LENGTHS],
        "semantic_m_tokens": [[lib.at_w2vbert_num_tokens(n, m) for m in M_PADS] for n in M_LENGTHS],
        "semantic_s_workspace": [[lib.at_hubert_workspace_bytes(None, b, n) for b in BATCHES] for n in S_LENGTHS],
        "semantic_s_tokens": [lib.at_hubert_num_tokens(n) for n in S_LENGTHS],
    }


# recorded at commit d77eef4 (the last one with each encode body as one function)
EXPECTED = {
    'semantic_m_tokens': [[0, 0], [1, 4], [2, 4], [32, 32], [33, 36], [150, 152], [1749, 1752]],
    'semantic_m_workspace': [[[7168, 19456, 399616, 1873408], [7168, 19456, 399616, 1873408]],
                             [[9999872, 10073856, 12334080, 31044864], [10075392, 10300672, 17177088, 83630848]],
                             [[10035968, 10182912, 14665728, 51936000], [10086400, 10334208, 17894400, 86993152]],
                             [[11128320, 13461248, 154345472, 728475136], [11128320, 13461248, 154345472, 728475136]],
                             [[11165440, 13571072, 166638592, 749366528], [11240960, 13797888, 171481600, 811913984]],
                             [[15433472, 36337152, 728682752, 3394532864], [15483904, 36488448, 731911424, 3439551488]],
                             [[133451520, 400352000, 8441218048, 39537080320], [133527040, 400579328, 8446061056, 39599627776]]],
    'semantic_s_tokens': [0, 1, 3, 33, 256, 299],
    'semantic_s_workspace': [[0, 0, 0, 0], [11672064, 20071936, 276268288, 1274927360], [12206592, 21675520, 310478592, 1450230528],
                             [28088832, 69322496, 1386718464, 6476427008], [142790912, 428371200, 9138572288, 42837055744],
                             [170843648, 497587200, 10537973504, 49392546560]],
}


def test_every_plan_size_is_the_recorded_one():
    got = measure(_cabi.load())
    assert set(got) == set(EXPECTED)
    for name, want in EXPECTED.items():
        assert got[name] == want, name


def test_the_table_reaches_the_padding_and_the_row_tiles():
    """what makes the table worth pinning: the pad multiple changes the token count (and with it the plan) exactly where T is no multiple of 4, a clip
    one sample short of the first token plans no tokens, and the plans grow with the batch"""
    tok = dict(zip(M_LENGTHS, EXPECTED["semantic_m_tokens"]))
    assert tok[559] == [0, 0] and tok[560] == [1, 4] and tok[10480] == [32, 32] and tok[10800] == [33, 36] and tok[560000][0] == 1749
    for (t0, t4), (w0, w4) in zip(EXPECTED["semantic_m_tokens"], EXPECTED["semantic_m_workspace"]):
        assert (w0 == w4) == (t0 == t4)
        assert all(a < b for a, b in zip(w0, w0[1:])) and all(a < b for a, b in zip(w4, w4[1:]))
    assert EXPECTED["semantic_s_tokens"][:2] == [0, 1] and 256 in EXPECTED["semantic_s_tokens"]
    assert EXPECTED["semantic_s_workspace"][0] == [0, 0, 0, 0]
    for row in EXPECTED["semantic_s_workspace"][1:]:
        assert all(a < b for a, b in zip(row, row[1:]))
