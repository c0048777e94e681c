"""The JSGF scanner, parser and expander (csrc/ssw_jsgf.c) under AddressSanitizer + UBSan: a
stand-alone program (tests/harness/jsgf_asan_main.c, with its own main) built from the product's
host C sources.  It parses and expands every committed grammar, every line-end prefix of each, and
a fixed list of malformed and outsized inputs: unterminated tag, quote, comment and weight, an
empty rule, a stray ), nesting 200 and 5000 deep, 1 MB tokens, an empty string.  Nothing is loaded
into Python."""
import glob
import os
import subprocess

import pytest

from tests import jsgf_common as C
from tests.conftest import MODEL_ROOT, ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("jsgf_asan") / "jsgf_asan_main")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "harness", "jsgf_asan_main.c")]
    cmd += [os.path.join(CSRC, f) for f in ("ssw_model.c", "ssw_lexicon.c", "ssw_fsg.c",
                                            "ssw_jsgf.c")]
    cmd += ["-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_jsgf_code_is_clean_under_asan_ubsan(program):
    grammars = sorted(glob.glob(os.path.join(C.JSGF_DIR, "*.gram")))
    assert len(grammars) == len({c[2] for c in C.CASES})
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program, os.path.join(MODEL_ROOT, "en-us")] + grammars,
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok %d grammars" % len(grammars)), r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
