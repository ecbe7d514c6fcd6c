"""The acoustic workspace plans, pinned: the six size functions of the C ABI (pure host code, NULL handle, no device) against a table recorded
before the acoustic host code was split into encodec_plan.h / encodec_encode.hip / encodec_decode.hip. A plan is what a caller allocates from, so a
refactor of the host code must leave every figure as it was; the table is a literal so that the test passes on both sides of that change.

Encode: every length of tests/acoustic_routes.LENGTHS at B = 1, 3, 81 (one past the pipelined LSTM's 80 clips) and 300 (past the default
sub-batch of 256). Stream pushes of 320 / 2240 / 24000 samples, decode of 1 / 7 / 75 / 257 frames one-shot and streamed, the two state sizes.
"""
from audiotoken_amd import _cabi
from tests import acoustic_routes as AR

BATCHES = (1, 3, 81, 300)
PUSHES = (320, 2240, 24000)
DEC_FRAMES = (1, 7, 75, 257)


def measure(lib):
    """{name: [bytes per B of BATCHES] per input}, in the order of the module constants."""
    return {
        "encode": [[lib.at_encodec_workspace_bytes(None, b, n) for b in BATCHES] for n in AR.LENGTHS],
        "encode_stream": [[lib.at_encodec_stream_workspace_bytes(None, b, n) for b in BATCHES] for n in PUSHES],
        "decode": [[lib.at_encodec_decode_workspace_bytes(None, b, t) for b in BATCHES] for t in DEC_FRAMES],
        "decode_stream": [[lib.at_encodec_decode_stream_workspace_bytes(None, b, t) for b in BATCHES] for t in DEC_FRAMES],
        "encode_state": [lib.at_encodec_stream_state_bytes(None, b) for b in BATCHES],
        "decode_state": [lib.at_encodec_decode_stream_state_bytes(None, b) for b in BATCHES],
    }


# recorded at commit c5a7fb8 (the last one with all of this in encodec.hip)
EXPECTED = {'encode': [[7346944, 21292288, 573413376, 1837622528], [7346944, 21293056, 573438976, 1837704448], [7350528, 21303808, 573724160, 1838605568],
            [7350528, 21304320, 573749760, 1838687488], [7370496, 21362944, 575321088, 1843651840], [7370496, 21363712, 575346688, 1843733760],
            [7374080, 21374464, 575631872, 1844634880], [7374080, 21374976, 575657472, 1844716800], [7570944, 21964288, 591557376, 1894966528],
            [7570944, 21965056, 591582976, 1895048448], [7574528, 21975808, 591868160, 1895949568], [7574528, 21976320, 591893760, 1896031488],
            [7594496, 22034944, 593465088, 1900995840], [7594496, 22035712, 593490688, 1901077760], [7598080, 22046464, 593775872, 1901978880],
            [7598080, 22046976, 593801472, 1902060800], [8752384, 25508608, 683936256, 2190646528], [8752384, 25509376, 683961856, 2190728448],
            [8755968, 25520128, 684247040, 2191629568], [8755968, 25520640, 684272640, 2191711488], [8775936, 25579264, 685843968, 2196675840],
            [8775936, 25580032, 685869568, 2196757760], [8779520, 25590784, 686154752, 2197658880], [8779520, 25591296, 686180352, 2197740800],
            [8976384, 26180608, 702080256, 2247990528], [8976384, 26181376, 702105856, 2248072448], [8979968, 26192128, 702391040, 2248973568],
            [8979968, 26192640, 702416640, 2249055488], [8999936, 26251264, 703987968, 2254019840], [8999936, 26252032, 704013568, 2254101760],
            [9003520, 26262784, 704298752, 2255002880], [9003520, 26263296, 704324352, 2255084800], [15600384, 46052608, 1222699008, 3911245056],
            [16023808, 47322880, 1256332800, 4018287872], [19583744, 58002688, 1540706304, 4921509120], [20806656, 61671424, 1637107968, 5229159680],
            [21824256, 64724992, 1716899840, 5484315904], [23612672, 70090240, 1857780224, 5934028032], [24301824, 72157696, 1911610880, 6106389760],
            [30925312, 92028160, 2437496576, 7780343040], [25436928, 75563008, 2000905216, 6391577856], [26982144, 80198656, 2122749952, 6780384512],
            [29420288, 87513088, 2318912512, 7401841920], [30643200, 91181824, 2415314176, 7709492480], [31904000, 94964736, 2514141696, 8025554176],
            [33449216, 99600384, 2635986432, 8414360832], [34138368, 101667840, 2689817088, 8586722560], [21650944, 64205568, 1703550720, 5441383680],
            [92756992, 278260224, 7343011840, 23432541184], [92756992, 278260736, 7343037440, 23432623104],
            [98936320, 295274752, 7801733888, 24895327488], [98936320, 295275264, 7801759488, 24895409408]],
 'encode_stream': [[7879168, 22890240, 615906048, 1972665600], [9565696, 27949824, 748533504, 2396294400],
                   [32611840, 97088256, 2570149632, 8204053760]],
 'decode': [[2356480, 5486848, 126907648, 401001216], [4165888, 10915072, 271061248, 861592320], [27019520, 79475968, 2093598976, 6682196736],
            [90424576, 269691136, 7090554112, 22634482432]],
 'decode_stream': [[2969344, 7325440, 175222528, 557187840], [4794112, 12799744, 320620288, 1022386944], [27952896, 82276096, 2168661760, 6929556224],
                   [91692800, 273495808, 7191953152, 22987277056]],
 'encode_state': [23040, 69120, 1866240, 6912000],
 'decode_state': [15360, 46080, 1244160, 4608000]}


def test_every_plan_size_is_the_recorded_one():
    got = measure(_cabi.load())
    assert len(got["encode"]) == len(AR.LENGTHS) == 52
    for name, want in EXPECTED.items():
        assert got[name] == want, name
    assert set(got) == set(EXPECTED)


def test_the_table_reaches_the_sub_batch_and_the_pipe_limit():
    """what makes the table worth pinning: B = 300 plans a 256-clip sub-batch (less than 300 / 81 times the B = 81 conv stack), and B = 81 loses the
    pipelined LSTM's second gate buffer (less than 81 / 3 times B = 3 where the conv stack is small against it)"""
    for row in EXPECTED["encode"]:
        assert 0 < row[0] < row[1] < row[2] < row[3]
        assert row[3] * 81 < row[2] * 300
    one, three, big, _ = EXPECTED["decode"][DEC_FRAMES.index(257)]
    assert big * 3 < three * 81
