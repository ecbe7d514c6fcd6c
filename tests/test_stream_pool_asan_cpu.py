"""CPU: the host-side argument checks of the stream pool copies (csrc/stream_pool.hip: the slot list, the launcher's own checks) under AddressSanitizer, as
a stand-alone program with its own main (tools/stream_pool_args.hip, `make -C audiotoken_amd/csrc pool_asan`). Every case is refused before anything is
launched, so no device is needed; an AddressSanitizer report or a failed case ends the program with a non-zero status."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pool_argument_checks_under_address_sanitizer():
    out = subprocess.run(["make", "-C", os.path.join(ROOT, "audiotoken_amd", "csrc"), "pool_asan"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "stream pool argument checks: ok" in out.stdout
    assert "AddressSanitizer" not in out.stdout + out.stderr
