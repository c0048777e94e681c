"""The workspace layout builder (csrc/ssw_ws_layout.inc) on the CPU.

tests/harness/ws_layout_host.cpp includes the builder (plain C++17, no HIP header) and runs
layouts of 1 to 40 pieces with sizes drawn from {0, 1, 255, 256, 257, 4096} (fixed seed):
offsets against the rule of the hand-written piece tables it replaced, alignment, no overlap,
the total, and fill() from every piece boundary into a sentinel-filled buffer of exactly the
size it may write; then the same pieces registered with typed pointers: the offsets of the
plain calls, resolve() = base + offset for every pointer, a zero-byte optional table keeps its
slot.  Built with -fsanitize=address,undefined and run as a process of its own.
The rule is restated here too, over the offsets the program prints."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "harness", "ws_layout_host.cpp")


def test_layout_offsets_and_fill(tmp_path):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp_path / "ws_layout_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, SRC], check=True, cwd=str(tmp_path))
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1].startswith("ok: "), r.stdout[-2000:] + r.stderr[-2000:]
    n_layouts, n_pieces, n_fills = [int(x) for x in re.findall(r"\d+", lines[-1])]
    assert n_layouts == 40 * 5 and n_pieces == 5 * sum(range(1, 41)) and n_fills > n_pieces
    # every piece once more with a typed pointer, and the four of the optional-table case
    assert lines[-2].startswith("slots: "), r.stdout[-2000:]
    assert int(re.findall(r"\d+", lines[-2])[0]) == n_pieces + 4
    # the parent's rule: off = (off + bytes + 255) & ~255, a zero-byte piece takes no space
    seen = set()
    layouts = [ln for ln in lines if ln.startswith("L ")]
    assert len(layouts) == n_layouts
    for ln in layouts:
        body, total = ln[2:].split(" = ")
        off = 0
        pieces = [tuple(int(x) for x in p.split(":")) for p in body.split()]
        for i, (nbytes, got) in enumerate(pieces):
            assert got == off and got % 256 == 0, ln
            if i:
                assert pieces[i - 1][1] + pieces[i - 1][0] <= got, ln
            off = (off + nbytes + 255) & ~255
            seen.add(nbytes)
        assert int(total) == off, ln
    assert len({len(ln.split()) for ln in layouts}) == 40      # 1 .. 40 pieces
    assert seen == {0, 1, 255, 256, 257, 4096}
