"""tests/golden/fsg_default_results.json -- the reference library recognising against word FSGs
in its DEFAULT configuration (compallsen = no) -- beside fsg_results.json, the compallsen = yes
records: the same cases, the same words, other scores."""
import json
import os
import subprocess
import sys

import pytest

from tests import fsg_common as C
from tests.conftest import ROOT

DEFAULT_JSON = os.path.join(C.GOLD, "fsg_default_results.json")
GENERATOR = os.path.join(C.GOLD, "make_fsg_default.py")


def _default():
    with open(DEFAULT_JSON, encoding="utf-8") as f:
        return json.load(f)


def test_the_fixture_has_exactly_the_cases():
    fx = _default()
    assert sorted(fx) == sorted(c[0] for c in C.CASES)
    for name, group, grammar, model, recording, samples in C.CASES:
        rec = fx[name]
        assert (rec["group"], rec["grammar"], rec["model"], rec["recording"], rec["samples"]) \
            == (group, grammar, model, recording, samples)
    assert os.path.getsize(DEFAULT_JSON) < (1 << 20)


def test_same_words_frames_and_errors_other_scores():
    """what the issue's table says: the hypothesis text is the same wherever there is one, every
    hypothesis score and every segment list differs, the cases without a hypothesis are unchanged"""
    fx, yes = _default(), C.results()
    scored = 0
    for name in fx:
        a, b = fx[name], yes[name]
        assert a["hyp"] == b["hyp"], name
        assert a["frames"] == b["frames"], name
        assert a["errors"] == b["errors"], name
        assert a["fsg"] == b["fsg"] and a["fsg_search"] == b["fsg_search"], name
        if a["score"] is None:
            assert b["score"] is None and a["segments"] == b["segments"] == [], name
            continue
        scored += 1
        assert a["score"] != b["score"], name
        assert a["segments"] != b["segments"], name
        assert [s[0] for s in a["segments"]] == [s[0] for s in b["segments"]], name
    assert scored == 8


def test_the_scores_of_the_default_configuration():
    fx = _default()
    want = {"goforward": -3210, "loop": -4432, "nulls": -3125, "sil": -2436, "fr": -4427,
            "loop_1200ms": -1723, "loop50": -6324, "loop110": -6560}
    assert {k: v["score"] for k, v in fx.items() if v["score"] is not None} == want


def test_generator_check_mode_agrees_with_the_reference_build():
    from oracle import reference
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_ctypes_mirror_resolves_the_new_symbols():
    from soundswallower_amd import _lib
    _lib.build()
    L = _lib.lib()
    assert L.ssw_recognize_batch_active.argtypes is not None
    assert len(L.ssw_recognize_batch_active.argtypes) == 13
    assert L.ssw_grammar_active_stats.restype is not None
    import soundswallower_amd as ssw
    assert callable(ssw.recognize_batch_active) and callable(ssw.Model.grammar_active_stats)
