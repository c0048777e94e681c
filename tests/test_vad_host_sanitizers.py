"""The host path of voice activity detection (csrc/ssw_vad.c over csrc/ssw_vad_core.inc, the
arithmetic the kernel is built from) under AddressSanitizer + UBSan: a stand-alone program
(tests/harness/vad_host_main.c, with its own main) run as its own process over the degenerate
inputs -- digital silence, a full-scale square wave, noise of amplitude 3, a DC offset of 8000 --
and one recording, at the four rates the detector works at, in every mode and frame length, whole
and in pieces, with the endpointer's replay behind.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests import vad_common as V
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("vad_asan") / "vad_host_main")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, "-o", exe,
           os.path.join(ROOT, "tests", "harness", "vad_host_main.c"),
           os.path.join(CSRC, "ssw_vad.c"), os.path.join(CSRC, "ssw_model.c"), "-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("rate", (8000, 16000, 32000, 48000))
def test_vad_host_path_is_clean_under_asan_ubsan(program, tmp_path, rate):
    files = []
    for name in V.DEGENERATE + ("goforward",):
        path = str(tmp_path / (name + ".raw"))
        V.stream(name, rate)[:rate * 4 + 7].astype("<i2").tofile(path)   # 4 s and an odd tail
        files.append(path)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program, str(rate)] + files, capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d runs, " % (12 * len(files))), r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
