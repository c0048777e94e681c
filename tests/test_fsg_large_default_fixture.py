"""tests/golden/fsg_large_default_results.json -- the reference library in its DEFAULT
configuration (compallsen = no) against the grammars of more than 4096 phone-tree HMMs, written
by make_fsg_large_default.py -- beside fsg_large_results.json, the compallsen = yes records of the
same cases; and the plans ssw_grammar_prepare_large_active makes or refuses.  No device needed."""
import os
import subprocess
import sys

import pytest

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests import fsg_large_common as CL
from tests import fsg_large_default_common as CD
from tests.conftest import MODEL_ROOT, ROOT

GENERATOR = os.path.join(C.GOLD, "make_fsg_large_default.py")


@pytest.fixture(scope="module")
def host():
    """en-us model without a device + lexicon + the three grammars"""
    d = os.path.join(MODEL_ROOT, "en-us")
    m = ssw.Model(d, config={"device": -2})
    lex = ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    return m, lex, {g: ssw.Fsg.read(m, lex, C.fsg_path(g)) for g in CL.GRAMMARS}


def test_the_fixture_has_exactly_the_six_cases_and_the_default_scores():
    fx, yes = CD.results(), CL.results()
    assert len(CD.TRUTH) == 6 and sorted(fx) == sorted(CD.TRUTH) == sorted(c[0] for c in CL.CASES)
    for name, group, grammar, model, recording, samples in CL.CASES:
        rec = fx[name]
        assert (rec["group"], rec["grammar"], rec["model"], rec["recording"], rec["samples"]) \
            == (group, grammar, model, recording, samples)
        assert rec["frames"] == yes[name]["frames"] == (120 if samples else 279)
        assert (rec["hyp"], rec["score"]) == CD.TRUTH[name], name
        assert rec["errors"] == [] and rec["json"].endswith("\n")
        # the words and frames of the compallsen = yes record, other scores
        assert [s[:3] for s in rec["segments"]] == [s[:3] for s in yes[name]["segments"]], name
        assert rec["hyp"] == yes[name]["hyp"] and rec["score"] != yes[name]["score"], name
        assert rec["fsg"] == yes[name]["fsg"] and rec["fsg_search"] == yes[name]["fsg_search"], name
    assert os.path.getsize(CD.RESULTS_JSON) < (1 << 20)


def test_the_null_grammar_files_a_null_entry_after_every_word():
    fx = CD.results()
    for name in ("nulls200", "nulls200_1200ms"):
        words = [s[0] for s in fx[name]["segments"]]
        spoken = [i for i, w in enumerate(words) if w != "(NULL)" and not w.startswith("<")]
        assert len(spoken) >= 2 and all(words[i + 1] == "(NULL)" for i in spoken)


def test_generator_check_mode_agrees_with_the_reference_build():
    from oracle import reference
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_ctypes_mirror_resolves_the_new_symbols():
    from soundswallower_amd import _lib
    L = _lib.lib()
    assert len(L.ssw_grammar_prepare_large_active.argtypes) == 6
    assert L.ssw_grammar_prepare_large_active.restype is not None
    assert len(L.ssw_grammar_plan_active.argtypes) == 1
    assert L.ssw_grammar_plan_active(None) == -1


def test_a_flagged_plan_says_so_and_counts_the_reference_s_hmms(host):
    _, lex, fsgs = host
    for g, n in CL.HMMS.items():
        plan = lex.grammar_plan(fsgs[g], max_hmms=30000, active=True)
        assert plan.active is True and plan.hmms(0) == n, g
    assert lex.grammar_plan(fsgs["loop200"], max_hmms=30000).active is False
    assert lex.grammar_plan(ssw.Fsg.read(host[0], lex, C.fsg_path("goforward"))).active is False


def test_a_grammar_over_max_hmms_is_refused_under_the_new_name(host):
    _, lex, fsgs = host
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(fsgs["loop200"], max_hmms=5000, active=True)
    assert str(e.value) == ("ssw_grammar_prepare_large_active: grammar 0 (loop200) has 5613 "
                            "phone-tree HMMs: max_hmms allows at most 5000")
    with pytest.raises(ssw.SswError, match="bad arguments to ssw_grammar_prepare_large_active"):
        lex.grammar_plan(fsgs["loop200"], max_hmms=0, active=True)
    with pytest.raises(ssw.SswError, match=r"ssw_grammar_prepare_large_active: max_hmms = 30001: "
                                           r".* at most 30000"):
        lex.grammar_plan(fsgs["loop200"], max_hmms=30001, active=True)


def test_active_without_max_hmms_is_a_value_error(host, monkeypatch):
    """named in the message, and nothing is called"""
    _, lex, fsgs = host
    monkeypatch.setattr(ssw.api.GrammarPlan, "__init__",
                        lambda *a, **k: pytest.fail("a plan was made"))
    with pytest.raises(ValueError, match="max_hmms"):
        lex.grammar_plan(fsgs["loop200"], active=True)
