"""The front end's logarithm (csrc/ssw_fe_log.inc, what fe_cep_kernel takes of every mel value)
on the CPU: tests/harness/fe_log_host.cpp includes it as plain C++ (built with -ffp-contract=off
and UBSan, as a process of its own) and prints it for 30,000 arguments from a fixed generator;
every one must be the correctly rounded logarithm, which mpmath gives at 300 bits.

How often libm's own log differs is printed and bounded too: glibc states an error below 0.52
ulp, so it can miss the correctly rounded value only where the true value lies within 0.02 ulp of
the middle between two doubles, 4 % of arguments at the very most (it is a few in 100,000).

The test needs the correctly rounded logarithm: the file does not exist without it."""
import os
import shutil
import subprocess

import mpmath

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "fe_log_host.cpp")
N = 30000


def test_fe_log_is_correctly_rounded(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "fe_log_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-ffp-contract=off", "-fsanitize=undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe, str(N)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == N + 1 and lines[-1].startswith("glibc ")
    mpmath.mp.prec = 300
    bad = []
    for line in lines[:N]:
        x, y = (float.fromhex(t) for t in line.split())
        if float(mpmath.log(mpmath.mpf(x))) != y:
            bad.append(line)
    assert not bad, (len(bad), bad[:5])
    differ = int(lines[-1].split()[1])
    print("libm's log differs from the correctly rounded one at", differ, "of", N)
    assert differ <= 0.04 * N
