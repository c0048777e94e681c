"""The senone kernels' dynamic LDS carves (csrc/ssw_senone_lds.inc) on the CPU.

tests/harness/senone_lds_host.cpp includes the carve structs (plain C++17, no HIP header) beside a
verbatim copy of the typed-pointer carves of ptm_senone_kernel, ms_senone_kernel,
senone_active2_kernel and senone_listed_kernel and of the byte counts their launchers computed,
and compares every region offset and bytes() over fpb 1, 2 x n_cb 1, 7, 8, 9, 36, 42, 64 x
n_feat 1, 3, 4 x ms x cap 1, 2, 63, 64, 65, 449, 5126 x n_sen 1, 2107, 2108, 5126 x full (each
carve over the parameters it has; the per-wave carves for each of the four waves), and
FpaPlanCarve against fpa_plan_kernel's pointer steps and the host's byte count over nw32 1, 2, 63,
64, 65, 66, 161, 2048 x cap 2, 3, 64, 65, 66, 448, 449, 450, 5126, 65534 (odd ones included:
the list then ends 2-aligned, which is why fpa_cap hands out even capacities only).  It also
asserts that no two regions of a carve overlap, that the last ends inside bytes(), and that every
region is aligned as its element type needs.  Built with -fsanitize=address,undefined and run as a
process of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "senone_lds_host.cpp")


def test_carves_equal_the_formulas_they_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "senone_lds_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    n_cb_feat, n_cap, n_sen, waves = 7 * 3, 7, 4, 4
    per_scorer = 2 + n_cap * waves + n_cap * n_sen * 2 * waves  # senone, listed, active2
    fpa_plan = 8 * 10 * waves  # nw32 x cap
    assert int(re.findall(r"\d+", last)[0]) == n_cb_feat * (1 + 2 * per_scorer) + fpa_plan
