"""The scan's selection network (csrc/ssw_top5_select.inc) against a full sort, on the CPU.

tests/harness/top5_select_host.cpp includes the network's own text with the three-input
operations written in plain C, and runs it on: every placement of the five largest of a lane's 64
keys within nine consecutive positions (one triple and its neighbours, across the leftover 16th
slot of a tile and across tile boundaries), strictly ascending and descending keys, keys that
differ in the label bits only, and 10^5 random draws (negative keys included).  Built with
-fsanitize=address,undefined and run as a process of its own."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "top5_select_host.cpp")


def test_selection_network_equals_full_sort(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "top5_select_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-Wno-unknown-pragmas",     # the network's "#pragma unroll"
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout + r.stderr
    # 64 windows x 9 * 8 * 7 * 6 * 5 ordered placements, and the rest
    n_cases, n_placed = [int(x) for x in re.findall(r"\d+", r.stdout)[:2]]
    assert n_placed == 64 * 15120 and n_cases >= n_placed + 100000
