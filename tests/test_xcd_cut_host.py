"""The matrix-core scan's XCD cut (csrc/ssw_xcd_cut.inc) on the CPU.

tests/harness/xcd_cut_host.cpp includes the cut (plain C++17, no HIP header) beside a verbatim
copy of the loop it was moved out of and compares all ten ints for n_cbf in {1, 3, 7, 126} x
tile_groups in {1, 2, 5, 64} x both balance modes, on seeded random exact-list counts 0 .. 128
and on all-zero and all-equal ones.  Built with -fsanitize=address,undefined and
-ffp-contract=off (as the library is: the cut compares sums of doubles) and run as a process
of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "xcd_cut_host.cpp")


def test_xcd_cut_equals_the_loop_it_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "xcd_cut_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-ffp-contract=off", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    assert int(re.findall(r"\d+", last)[0]) == 4 * 4 * 2 * 8
