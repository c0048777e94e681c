"""Words added to a loaded dictionary (csrc/ssw_lexicon.c: ssw_dict_add_word,
ssw_dict_lookup_word) under AddressSanitizer + UBSan: a stand-alone program
(tests/harness/dict_add_host.c, with its own main) built from the product's host C sources.  It
loads en-us, adds words and alternates, is refused everything the call refuses, looks words up into
buffers of every length, then adds 9000 words to a small dictionary, past two capacity doublings
and their rehashes, and frees everything.  Nothing is loaded into Python.

The test needs the feature: the program does not link without ssw_dict_add_word."""
import os
import subprocess

import pytest

from tests.conftest import MODEL_ROOT, ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("dict_add_asan") / "dict_add_host")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "harness", "dict_add_host.c")]
    cmd += [os.path.join(CSRC, f) for f in ("ssw_model.c", "ssw_lexicon.c", "ssw_fsg.c",
                                            "ssw_jsgf.c")]
    cmd += ["-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_dictionary_adds_are_clean_under_asan_ubsan(program, tmp_path):
    small = tmp_path / "small.dict"
    small.write_text("go G OW\nforward F AO R W ER D\nten T EH N\nmeters M IY T ER Z\n",
                     encoding="utf-8")
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program, os.path.join(MODEL_ROOT, "en-us"), str(small)],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # 6 + 9000 + 18 added; 12 + 9 refused; the small dictionary began with 4 + 5 (noisedict) words
    assert r.stdout == "ok 9024 added, 21 refused, 9027 words\n", r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
