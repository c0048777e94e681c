"""The scan's two-level selection network, its fold and its merge by position
(csrc/ssw_top5_select.inc: ssw_top5_tile2, ssw_top5_fold2, ssw_top5_insert_from, ssw_top5_merge)
against a full sort and against the one-level network, on the CPU.

tests/harness/top5_select2_host.cpp includes the network's own text with the three-input
operations written in plain C, and runs it on: every placement of the five largest of a lane's 64
keys within nine consecutive positions (all 64 starts); the five largest on every 5 of the 16
positions of one tile (the second-level triples span the tile, the leftover 16th key included),
24 orders of each of the 4,368 sets in each of the four tiles; keys that differ in the label
bits only; 10^5 random draws (wide, narrow, negative only); and whole frames of 128 keys whose
two lists are merged by position, either into the other.  Built with -fsanitize=address,undefined
and run as a process of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "top5_select2_host.cpp")


def test_two_level_network_equals_full_sort_and_one_level(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "top5_select2_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-Wno-unknown-pragmas",     # the network's "#pragma unroll"
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok: "), r.stdout + r.stderr
    n_cases, n_placed, n_tile, n_merges = [int(x) for x in re.findall(r"\d+", r.stdout)[:4]]
    # 64 windows x 9 * 8 * 7 * 6 * 5 ordered placements; 4 tiles x C(16, 5) sets x 24 orders,
    # at least 10^5 per tile; the random draws; two lists per merged frame
    assert n_placed == 64 * 15120
    assert n_tile == 4 * 4368 * 24 and n_tile // 4 >= 100000
    assert n_merges >= 40000
    assert n_cases >= n_placed + n_tile + 100000 + 2 * n_merges
