"""The loader of single-codebook models (csrc/ssw_model.c) under AddressSanitizer + UBSan: a
stand-alone program (tests/harness/sc_loader_main.c, with its own main) built from ssw_model.c.  It
loads models A and B and the files the loader has to refuse -- among them the stream of 20
dimensions in a model of 42 codebooks, whose records used to be written before the length was
checked.  Nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests import sc_common as S
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("sc_asan") / "sc_loader_main")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "harness", "sc_loader_main.c"),
           os.path.join(CSRC, "ssw_model.c"), "-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_single_codebook_loader_is_clean_under_asan_ubsan(program, tmp_path):
    tmp = str(tmp_path)
    args = ["ok", S.model_a_dir(os.path.join(tmp, "A")), "4",
            "ok", S.model_a_ties_dir(os.path.join(tmp, "A-ties")), "1",
            "ok", S.model_b_dir(os.path.join(tmp, "B")), "4"]
    refused = S.refused_models(tmp)
    for name in sorted(refused):
        d, topn, words = refused[name]
        args += ["bad", d, str(topn), words[-1]]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 3 loaded, %d refused" % len(refused)), r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
