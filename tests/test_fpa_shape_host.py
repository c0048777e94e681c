"""The default-configuration loop's shape and round policy (csrc/ssw_fpa_shape.inc) on the CPU.

tests/harness/fpa_shape_host.cpp includes fpa_shape, fpa_compare_slices, fpa_one_by_one and
fpa_next_only (plain C++17, no HIP header) beside a verbatim copy of the arithmetic of fpa_run
they were moved out of and compares every output -- the per-utterance mask offsets and their
total, max_nodes, the longest utterance, cap, the LDS bytes of the plan kernel and of the listed
scorer, the 156 KB refusal with its message, the utterance-start words and their bytes, the
comparison's slices -- over batches of 1, 4, 5, 16, 17 utterances x node counts 1, 63, 64, 65,
128, 129 from six starting points x four frame patterns (short; one utterance of 0 frames;
n_frames = 0; 100,000 frames each) x six senone counts (cap bound by n_sen, by the HMMs with an
odd and an even sum, the bitmap alone beyond a CU) x PTM, ms, continuous x four bounds on the
HMMs (none, 200, the last one accepted and the first one refused at 156 KB) x the carry on and
off; and the two decisions of the round policy for SSW_FPA_SUB -1, 0, 1 x the same batch sizes x
0, 1, 4, 5, n / 4, n / 4 + 1, n - 1 and n unproven utterances.  Built with
-fsanitize=address,undefined and run as a process of its own."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "fpa_shape_host.cpp")


def test_fpa_shape_equals_the_arithmetic_it_replaced(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "fpa_shape_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    last = r.stdout.splitlines()[-1]
    assert last.startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    n_cases, n_refused, n_policy = [int(x) for x in re.findall(r"\d+", last)]
    batches, kinds, bounds, carry = 5 * 6 * 4, 3, 4, 2
    assert n_cases == batches * 6 * kinds * bounds * carry
    # 1,300,000 senones: every bound; 65,000: each kind at its own first refused bound (the
    # harness checks that every kind was accepted just under it)
    assert n_refused == batches * kinds * carry * (bounds + 1)
    assert n_policy == 3 * 5 * 8
