"""The folded log-add table of the batch senone kernel (csrc/ssw_senone_lds.inc) on the CPU.

ptm_senone_kernel's chain step is x + H[x - y] with H[d] = Hb - tab[|d|] - max(d, 0) one byte per
entry, Hb = max over 0 <= d <= wmax of d + tab[d] (wmax = the largest mixture-weight byte).
tests/harness/senone_fold_host.cpp includes the builder the host uploads the table with (plain
C++17, no HIP header) and

  - writes the table for the log-add tables of en-us and fr-fr (wmax of their mixture weights, and
    255), PTM (1,024 bytes around 512) and ms (2,048 around 1,024): compared here with the formula
    entry by entry, every entry a byte, Hb = 158 for the shipped models;
  - reports Hb for a made-up table whose entries do not fall fast enough: 256, which is what
    launch_senone refuses and what sends the ms scorer to ms_senone_kernel;
  - runs the kernel's chain arithmetic, restated with the same 32-bit and packed 16-bit operations,
    against the reference's step over the extremes (weights 0 and wmax side by side, relative
    scores 0 and the clamp, the ms accumulator starting below zero) and two million random slot
    pairs, with the fold's range claims as assertions.

Built with -fsanitize=address,undefined and run as a process of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import soundswallower_amd as ssw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "senone_fold_host.cpp")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    d = tmp_path_factory.mktemp("fold")
    out = str(d / "senone_fold_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", out, SRC], check=True, cwd=str(d))
    return out


@pytest.fixture(scope="module")
def shipped():
    """{name: (log-add table uint8 [256], largest mixture-weight byte)}"""
    got = {}
    for name in ("en-us", "fr-fr"):
        m = ssw.Model(ssw.model_dir(name), config={"device": ssw.SSW_DEVICE_NONE})
        got[name] = (m.table("logadd8").astype(np.uint8).copy(), int(m.table("ptm_mixw").max()))
        m.close()
    return got


def _run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _formula(tab, wmax, size):
    t = np.zeros(4096, np.int64)
    t[:256] = tab
    hb = max(int(t[:256].max()), int((np.arange(wmax + 1) + t[:wmax + 1]).max()))
    d = np.arange(size) - size // 2
    h = hb - t[np.abs(d)] - np.maximum(d, 0)
    h[d > wmax] = hb          # no chain gets there
    return hb, h


@pytest.mark.parametrize("name", ["en-us", "fr-fr"])
def test_table_is_the_formula_in_bytes(exe, shipped, tmp_path, name):
    tab, wmax = shipped[name]
    tabfile = str(tmp_path / "tab")
    tab.tofile(tabfile)
    assert wmax == 158
    for w in (wmax, 255):
        for size in (1024, 2048):
            out = str(tmp_path / f"out{w}_{size}")
            last = _run(exe, "table", tabfile, w, size, out)[-1]
            hb, h = _formula(tab, w, size)
            assert last == f"hb {hb}" and hb == w          # tab[w] = 0: Hb = wmax
            assert h.min() >= 0 and h.max() == hb <= 255
            got = np.fromfile(out, np.uint8)
            assert np.array_equal(got, h)
            # what the kernel relies on: x + H[d] = min(x, y) - tab[|d|] + Hb for every d in reach
            d = np.arange(-(size // 2), w + 1)
            t = np.zeros(4096, np.int64)
            t[:256] = tab
            assert np.array_equal(got[d + size // 2].astype(np.int64) - hb, -t[np.abs(d)] - np.maximum(d, 0))


def test_a_table_that_does_not_fold_into_bytes_is_reported(exe, tmp_path):
    """tab[250] = 6: Hb = 256 at wmax = 255 -- the condition launch_senone refuses a model on and
    ms_takes_packed_kernel leaves the packed kernel on; at wmax = 158 the same table folds."""
    tab = np.zeros(256, np.uint8)
    tab[:29] = [7, 6, 6, 5, 5, 5, 4, 4, 4, 3, 3, 3, 3, 2, 2, 2, 2, 2] + [1] * 11
    tab[250] = 6
    tabfile, out = str(tmp_path / "tab"), str(tmp_path / "out")
    tab.tofile(tabfile)
    assert _run(exe, "table", tabfile, 255, 1024, out)[-1] == "hb 256"
    assert not os.path.exists(out)
    assert _run(exe, "table", tabfile, 158, 1024, out)[-1] == "hb 158"
    assert os.path.getsize(out) == 1024


@pytest.mark.parametrize("ms", [0, 1], ids=["ptm", "ms"])
@pytest.mark.parametrize("wmax", [158, 255])
def test_folded_chain_equals_the_reference_step(exe, shipped, tmp_path, wmax, ms):
    tab, _ = shipped["en-us"]
    tabfile = str(tmp_path / "tab")
    tab.tofile(tabfile)
    lines = _run(exe, "chains", tabfile, wmax, ms)
    assert lines[-1].startswith("ok: "), lines[-3:]
    assert int(lines[-1].split()[1]) == 2000000 + 2048 * 2 * (11 if ms else 1)
