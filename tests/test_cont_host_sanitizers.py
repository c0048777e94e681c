"""The loader of continuous-density models (csrc/ssw_model.c) under AddressSanitizer + UBSan: a
stand-alone program (tests/harness/cont_loader_main.c, with its own main) built from ssw_model.c.
It loads model C1 and a synthetic model without an mdef, and three malformed sets of files:
truncated mixture weights, densities over the cap, one codebook more than there are senones.
Nothing is loaded into Python."""
import os
import subprocess

import pytest

from tests import cont_common as CC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("cont_asan") / "cont_loader_main")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "harness", "cont_loader_main.c"),
           os.path.join(CSRC, "ssw_model.c"), "-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_continuous_loader_is_clean_under_asan_ubsan(program, tmp_path):
    tmp = str(tmp_path)
    from soundswallower_amd import _lib
    _lib.build()  # (C1 is cut from en-us's tables, read through the library)
    c1 = CC.model_c1_dir(os.path.join(tmp, "C1"))
    syn = CC.synthetic_dir(os.path.join(tmp, "syn"), 65, (3, 64), 5, 11)
    cut = CC.synthetic_dir(os.path.join(tmp, "cut"), 65, (3,), 5, 12)
    p = os.path.join(cut, "mixture_weights")
    blob = open(p, "rb").read()
    with open(p, "wb") as fh:
        fh.write(blob[:len(blob) // 2])
    d65 = CC.synthetic_dir(os.path.join(tmp, "d65"), 4, (3,), 65, 13)
    cb5 = CC.synthetic_dir(os.path.join(tmp, "cb5"), 4, (3,), 2, 14, n_cb=5)
    args = ["ok", c1, "4", "ok", c1, "0", "ok", syn, "2",
            "bad", cut, "4", "mixture_weights",
            "bad", d65, "4", "65 densities",
            "bad", cb5, "4", "5 codebooks for 4 senones"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program] + args, capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok 3 loaded, 3 refused"), r.stdout
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
