"""CPU: the acoustic encoder's route function (csrc/encodec_plan.h, enc_route: pure host code) gives, for every clip length of the route table, the
signature that tests/acoustic_routes.py derives from the five documented predicates; the program also checks dec_route's and lstm_route's defaults and
that a carried state with lstm_f16x2 = 0 takes the fp32 recurrence. A stand-alone program with its own main
(tools/acoustic_route_check.hip, `make -C audiotoken_amd/csrc route_asan`) under AddressSanitizer and UndefinedBehaviorSanitizer; no device is needed."""
import os
import subprocess

from tests import acoustic_routes as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_enc_route_is_the_documented_signature_on_every_length():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "route_asan", "ROUTE_LENGTHS=" + " ".join(map(str, AR.LENGTHS))],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "acoustic route checks: ok" in out.stdout
    assert "Sanitizer" not in out.stdout + out.stderr and "runtime error" not in out.stdout + out.stderr
    rows = [tuple(map(int, ln.split())) for ln in out.stdout.splitlines() if ln[:1].isdigit()]
    assert [r[0] for r in rows] == list(AR.LENGTHS)
    for n, *sig in rows:
        assert tuple(sig) == AR.signature(n), n
    assert len({r[1:] for r in rows}) == 32
