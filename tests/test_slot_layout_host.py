"""The senone kernels' slot layout (csrc/ssw_slot_layout.inc) on the CPU.

tests/harness/slot_layout_host.cpp includes the builder (plain C++17, no HIP header) and checks
both layouts of the shipped models' sen2cb tables and of synthetic ones -- one codebook, every id
isolated, runs of every length 1..9, codebooks with no senone, seeded random ones: every senone
exactly once, groups in codebook order with ascending ids, the dense layout equal to the loop it
replaced, every quad of the prefix layout s0 .. s0 + n - 1 followed by padding with n as the
table says, padding only where a run of consecutive ids ends, and the rule that chooses between
the layouts.  Built with -fsanitize=address,undefined and run as a process of its own."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests.conftest import MODEL_ROOT, ROOT

SRC = os.path.join(ROOT, "tests", "harness", "slot_layout_host.cpp")


@pytest.fixture(scope="module")
def tables(tmp_path_factory):
    """table name -> the harness's figures for it"""
    _lib.build()
    tmp = tmp_path_factory.mktemp("slot_layout")
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    exe = str(tmp / "slot_layout_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, SRC],
                   check=True, cwd=str(tmp))
    args = []
    for name in ("en-us", "fr-fr"):
        m = ssw.Model(os.path.join(MODEL_ROOT, name), config={"device": -2})
        path = str(tmp / (name + ".sen2cb"))
        np.ascontiguousarray(m.table("sen2cb"), dtype="<i2").tofile(path)
        args += [name, str(m.n_cb), path]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok: %d tables" % (len(lines) - 1), r.stdout[-2000:]
    out = {}
    for ln in lines[:-1]:
        w = ln.split()
        assert w[0] == "table", ln
        out[w[1]] = {w[k]: int(w[k + 1]) for k in (2, 4, 6, 8)}
        out[w[1]]["shape2"] = (int(w[11]), int(w[12]))
        out[w[1]]["shape1"] = (int(w[14]), int(w[15]))
    return out


def test_every_table_passes_the_harness(tables):
    assert len(tables) == 2 + 4 + 24
    for name in ("one-codebook", "isolated", "runs-1-9", "empty-codebooks"):
        assert name in tables


def test_shipped_models_take_the_prefix_layout_at_the_same_group_shape(tables):
    """The figures DESIGN.md section 3 quotes: a few quads more, the workgroups' shape as before
    (en-us: 3 quads per thread and 448 threads at two frames per group)."""
    en, fr = tables["en-us"], tables["fr-fr"]
    assert (en["dense"], en["prefix"], en["short"], en["fits"]) == (1296, 1308, 71, 1)
    assert (en["shape2"], en["shape1"]) == ((3, 448), (2, 704))
    assert (fr["dense"], fr["prefix"], fr["short"], fr["fits"]) == (539, 550, 62, 1)
    assert (fr["shape2"], fr["shape1"]) == ((2, 320), (1, 576))


def test_scattered_ids_keep_the_dense_layout(tables):
    """Every id a run of its own: four times the slots, a larger workgroup -- the rule refuses."""
    iso = tables["isolated"]
    assert iso["prefix"] == 4000 and iso["dense"] == 1000 and iso["short"] == 4000
    assert iso["fits"] == 0
    assert tables["one-codebook"]["fits"] == 1
    assert tables["one-codebook"]["prefix"] == tables["one-codebook"]["dense"] == 1025
