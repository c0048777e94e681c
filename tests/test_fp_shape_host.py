"""The first pass's launch shape (csrc/ssw_fp_shape.inc) on the CPU.

tests/harness/fp_shape_host.cpp includes fp_shape (plain C++17, no HIP header) beside a verbatim
copy of the sizing loops and the kernel choice chain it was moved out of and compares every
output -- the per-utterance history and HBM-workspace offsets, their totals, `big`, `band`, the
band, the kernel instance, threads per block, LDS bytes, whether the mask is cleared first, and
the 2^31 refusal with its message -- over 14 batches of synthetic offset tables (node counts at
256/257, 512/513, 1024/1025; LDS sizes around 160 * 1024 - 512 bytes; an utterance of 0 frames;
fewer and more word-final HMMs than the band; 1 x and 2 x frames at the 2^31 boundary) x levels
0, 1, 2 x the kernel forced big or not x four window and four big threads-per-block knob values
x three history bands x `runs` all / some / none x export on / off.  Built with
-fsanitize=address,undefined and run as a process of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "fp_shape_host.cpp")


def test_fp_shape_equals_the_loops_it_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "fp_shape_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    n_cases, n_refused = [int(x) for x in re.findall(r"\d+", last)]
    assert n_cases == 14 * 3 * 2 * 4 * 4 * 3 * 3 * 2
    # the two batches beyond the boundary, whenever their last utterance is searched
    assert n_refused == 2 * 3 * 2 * 4 * 4 * 3 * 2 * 2
