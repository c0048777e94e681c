"""The continuous-density fixtures (tests/golden/cont_results.json, cont/rows.npz): the numpy
restatement of compute_dist / senone_eval (tests/cont_common.py) reproduces every row the
reference recorded -- only then is it a yardstick for the shapes the reference cannot load
(tests/test_gpu_cont.py) --, the generated model files are the same on every build, and
make_cont.py --check agrees where the reference build exists."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from tests import cont_common as CC
from tests.conftest import ROOT

NONE = {"device": ssw.SSW_DEVICE_NONE}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("cont_fx"))
    return {n: b(os.path.join(tmp, n)) for n, b in CC.BUILDERS.items()}


@pytest.fixture(scope="module")
def fx():
    return CC.results()


def test_fixture_holds_every_case(fx):
    assert sorted(fx["scoring"]) == sorted(CC.CASES)
    for case, rec in fx["scoring"].items():
        assert rec["scorer"] == "ms" and rec["frames"] == 278 == len(rec["row_crc"]), case
        assert sorted(rec["rows"], key=int) == ["0", "1", "2", "277"], case
    assert sorted(fx["rec"]) == ["goforward", "loop", "nulls"]
    assert all(r["scorer"] == "ms" and r["hyp"] for r in fx["rec"].values())
    assert fx["align"]["scorer"] == "ms" and fx["scale"] >= 40


@pytest.mark.parametrize("case", sorted(CC.CASES))
def test_restatement_reproduces_the_reference(dirs, fx, case):
    model, topn, aw, mixwfloor, scale = CC.CASES[case]
    rec = fx["scoring"][case]
    m = ssw.Model(**CC.model_paths(dirs[model]),
                  config=dict(NONE, topn=topn, aw=aw, mixwfloor=mixwfloor))
    feats = CC.features() * np.float32(fx["scale"] if scale != 1 else 1)
    rows = CC.score_in_pieces(CC.restated_from_model(m, aw=aw), feats)
    got = CC.row_crcs(rows)
    bad = [t for t in range(len(got)) if got[t] != rec["row_crc"][t]]
    assert not bad, "frames %s ... differ from the reference's" % bad[:8]
    for t, row in rec["rows"].items():
        assert np.array_equal(rows[int(t)], np.array(row, np.int16)), t


def test_the_order_rule_decides_in_the_ties_model(fx):
    """density 6 is density 2 again with another weight: were equal scores listed lower index
    first, other rows would come out"""
    assert fx["scoring"]["C3-ties"]["row_crc"] != fx["scoring"]["C3"]["row_crc"]


def _digest(d):
    h = hashlib.sha256()
    for n in sorted(os.listdir(d)):
        with open(os.path.join(d, n), "rb") as fh:
            h.update(n.encode() + b"\0" + fh.read())
    return h.hexdigest()


def test_generated_models_are_byte_identical_across_builds(dirs, tmp_path):
    CC._C3_CACHE.clear()  # (from en-us again, not from the first build's tables)
    for n, b in CC.BUILDERS.items():
        assert _digest(b(str(tmp_path / n))) == _digest(dirs[n]), n


def test_make_cont_check_agrees_with_the_reference_build():
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_cont.py"),
                        "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
