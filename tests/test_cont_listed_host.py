"""What the listed-senone kernel of continuous models (csrc/ssw_k11_cont.inc, cont_listed_kernel)
takes from the host, on the CPU: tests/harness/cont_listed_host.cpp, a stand-alone program with
its own main, built with -fsanitize=address,undefined from that file and csrc/ssw_model.c and run
as a process of its own (nothing is loaded into Python).

  table   ssw_host_build_cont_sm: the senone-major table holds exactly the floats of the mean, var
          and det tables, for (70 senones, streams 13 13 13, 8 densities) and (5, 1, 1)
  select  cont_select_rank, the selection the kernel includes (csrc/ssw_cont_select.inc), against
          the sequential cont_insert, exhaustively: 1 to 5 densities with distances from
          {WORST_DIST - 2^8, WORST_DIST, 0, 1, NaN}, topn 1 to 5, slot for slot
  rows    cont_active_rows (csrc/ssw_active_set.inc), the bitmap rows of the alignment path,
          against a frame-by-frame restatement of the active set and its bridges"""
import os
import re
import shutil
import subprocess

import pytest

from tests import cont_common as CC
from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cont_listed_host")
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no C++ compiler"
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-ffp-contract=off", "-O1", "-g"]
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + CSRC]
    obj, exe = str(tmp / "ssw_model.o"), str(tmp / "cont_listed_host")
    for cmd in (["gcc", "-std=gnu99", "-Wall"] + san + inc + ["-c", "-o", obj, os.path.join(CSRC, "ssw_model.c")],
                [cxx, "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas",
                 "-Wno-unused-function"] + san + inc
                + ["-o", exe, os.path.join(ROOT, "tests", "harness", "cont_listed_host.cpp"), obj,
                   "-lm", "-lpthread"]):
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    return exe


def _run(program, args):
    r = subprocess.run([program] + args, capture_output=True, text=True, env=ENV, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    return r.stdout


def test_senone_major_table_holds_the_floats_of_the_model(program, tmp_path):
    a = CC.synthetic_dir(str(tmp_path / "a"), 70, (13, 13, 13), 8, 21)
    b = CC.synthetic_dir(str(tmp_path / "b"), 5, (1,), 1, 22)
    out = _run(program, ["table", a, "4", "table", b, "1"])
    assert len(re.findall(r"^ok table ", out, re.M)) == 2, out
    assert "70 senones, 3 streams, 8 densities, 648 floats" in out, out
    assert "5 senones, 1 streams, 1 densities, 4 floats" in out, out   # (3, padded to 4)


def test_rank_selection_equals_sequential_insertion_exhaustively(program):
    out = _run(program, ["select"])
    # 5 topn x (5 + 25 + 125 + 625 + 3125) draws
    assert out.startswith("ok select: %d cases" % (5 * 3905)), out


def test_alignment_bitmap_rows_under_sanitizers(program):
    out = _run(program, ["rows"])
    m = re.match(r"ok rows: (\d+) utterances, (\d+) frames", out)
    assert m and int(m.group(1)) == 48 and int(m.group(2)) > 500, out
