"""tests/golden/cont_default_results.json -- the reference library recognising and aligning with
the continuous models C3 and C1 in its DEFAULT configuration (compallsen = no) -- is well-formed,
holds results only, and is what tests/golden/make_cont_default.py records."""
import json
import os
import subprocess
import sys

import pytest

from tests import cont_common as CC
from tests.conftest import ROOT

RESULTS_JSON = os.path.join(CC.GOLD, "cont_default_results.json")
GENERATOR = os.path.join(CC.GOLD, "make_cont_default.py")
GRAMMARS = ("goforward", "loop", "loop400", "nulls", "turtle")


def _fx():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)


def test_the_fixture_has_exactly_the_records():
    fx = _fx()
    assert sorted(fx) == ["C1", "C3"]
    assert os.path.getsize(RESULTS_JSON) < (1 << 18)
    for m, rec in fx.items():
        assert sorted(rec) == ["align", "rec", "rec_align"], m
        assert tuple(sorted(rec["rec"])) == GRAMMARS, m
        for g, r in rec["rec"].items():
            assert sorted(r) == ["errors", "frames", "hyp", "json", "score", "segments"], (m, g)
            assert r["frames"] == 279 and r["json"].endswith("\n"), (m, g)
            assert (r["hyp"] is None) == (r["score"] is None), (m, g)
            if r["hyp"] is None:
                assert r["segments"] == [] or r["errors"], (m, g)
            else:
                assert all(len(s) == 6 and isinstance(s[0], str) for s in r["segments"]), (m, g)
                words = [s[0] for s in r["segments"] if not s[0].startswith(("<", "(NULL)"))]
                assert " ".join(words) == r["hyp"], (m, g)
                assert json.loads(r["json"])["t"] == r["hyp"], (m, g)
        for key in ("align", "rec_align"):
            a = rec[key]
            assert a["frames"] == 279 and a["json0"] is not None, (m, key)
            assert (a["json1"] is None) == (a["json2"] is None), (m, key)
            for level in "012":
                if a["json" + level] is not None:
                    json.loads(a["json" + level])
        assert sorted(rec["rec_align"]) == ["errors", "frames", "hyp", "json0", "json1", "json2", "score"]


def test_the_default_configuration_is_not_the_whole_row_one():
    """the same words as compallsen = yes recorded for C3 (tests/golden/cont_results.json), other
    scores: the normaliser is the best LISTED senone"""
    fx, yes = _fx()["C3"]["rec"], CC.results()["rec"]
    for g in ("goforward", "loop", "nulls"):
        assert fx[g]["hyp"] == yes[g]["hyp"], g
        assert fx[g]["score"] != yes[g]["score"], g


def test_generator_check_mode_agrees_with_the_reference_build():
    from oracle import reference
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr
