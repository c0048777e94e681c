"""Grammars of more than 4096 phone-tree HMMs on the host: the fixture the reference library
recorded for them (tests/golden/fsg_large_results.json, written by make_fsg_large.py) and the
plans ssw_grammar_prepare_large makes or refuses.  No device needed."""
import os
import re
import subprocess
import sys

import pytest

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests import fsg_large_common as CL
from tests.conftest import MODEL_ROOT, ROOT

GENERATOR = os.path.join(C.GOLD, "make_fsg_large.py")


@pytest.fixture(scope="module")
def host():
    """en-us model without a device + lexicon + the three grammars"""
    d = os.path.join(MODEL_ROOT, "en-us")
    m = ssw.Model(d, config={"device": -2})
    lex = ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    return m, lex, {g: ssw.Fsg.read(m, lex, C.fsg_path(g)) for g in CL.GRAMMARS}


def test_the_fixture_has_exactly_the_six_cases_and_the_reference_scores():
    fx = CL.results()
    assert len(CL.CASES) == 6 and sorted(fx) == sorted(c[0] for c in CL.CASES)
    for name, group, grammar, model, recording, samples in CL.CASES:
        rec = fx[name]
        assert (rec["group"], rec["grammar"], rec["model"], rec["recording"], rec["samples"]) \
            == (group, grammar, model, recording, samples)
        assert rec["frames"] == (120 if samples else 279)
        assert (rec["hyp"], rec["score"]) == CL.TRUTH[name], name
        assert rec["errors"] == [] and rec["json"].endswith("\n")
    assert os.path.getsize(CL.RESULTS_JSON) < (1 << 20)


def test_the_null_grammar_files_a_null_entry_after_every_word():
    fx = CL.results()
    for name in ("nulls200", "nulls200_1200ms"):
        words = [s[0] for s in fx[name]["segments"]]
        spoken = [i for i, w in enumerate(words) if w != "(NULL)" and not w.startswith("<")]
        assert len(spoken) >= 2 and all(words[i + 1] == "(NULL)" for i in spoken)


def test_the_grammars_are_the_rule_s():
    for g, (n, _, states) in CL.GRAMMARS.items():
        name, n_states, start, final, trans = C.parse_fsg(C.fsg_path(g))
        words = [t[3] for t in trans if t[3] is not None]
        assert (name, n_states, start, final) == (g, states, 0, states - 1)
        assert words[:6] == "go forward ten meters backward nine".split()
        assert len(words) == len(set(words)) == (395 if g == "loop400" else n)
        with open(C.fsg_path(g), encoding="utf-8") as f:
            assert f.readline().startswith("#")
        assert os.path.getsize(C.fsg_path(g)) < (1 << 20)


def test_generator_check_mode_agrees_with_the_reference_build():
    from oracle import reference
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_plan_counts_the_reference_s_hmms(host):
    """fsg_lextree_n_pnode of the reference for the three grammars; built on the host"""
    _, lex, fsgs = host
    for g, n in CL.HMMS.items():
        assert lex.grammar_plan(fsgs[g], max_hmms=30000).hmms(0) == n, g
    plan = lex.grammar_plan([fsgs["loop200"], fsgs["loop400"]], max_hmms=12000)
    assert [plan.hmms(i) for i in range(3)] == [5613, 11818, -1]


def test_a_grammar_over_max_hmms_is_refused_with_count_and_limit(host):
    _, lex, fsgs = host
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(fsgs["loop200"], max_hmms=5000)
    assert str(e.value) == ("ssw_grammar_prepare_large: grammar 0 (loop200) has 5613 phone-tree "
                            "HMMs: max_hmms allows at most 5000")


def test_max_hmms_over_the_ceiling_is_refused(host):
    _, lex, fsgs = host
    with pytest.raises(ssw.SswError, match=r"max_hmms = 30001: .* at most 30000"):
        lex.grammar_plan(fsgs["loop200"], max_hmms=30001)
    with pytest.raises(ssw.SswError, match="bad arguments to ssw_grammar_prepare_large"):
        lex.grammar_plan(fsgs["loop200"], max_hmms=0)


def _loop_over_dictionary_words(m, lex, lo, hi):
    words = [lex.word(i) for i in range(lo, hi)]
    words = [w for w in words if w and "(" not in w and not w.startswith("<")]
    return ssw.Fsg.create(m, lex, "big", 0, 0, [(0, 0, 1.0 / len(words), w) for w in words])


def test_the_3000_word_grammar_against_the_ceiling(host):
    """the grammar of test_fsg_host.test_grammar_over_the_hmm_limit_is_refused_by_the_plan has
    29652 phone-tree HMMs: within the ceiling, so a plan is made of it (on the host) and any
    lower max_hmms refuses it.  The same loop over 200 more dictionary entries is beyond 30000
    and is refused under the ceiling itself, the message naming 30000"""
    m, lex, _ = host
    f = _loop_over_dictionary_words(m, lex, 200, 3200)
    n = len(lex.grammar_graph(f)[0])
    assert 4096 < n <= 30000
    assert lex.grammar_plan(f, max_hmms=30000).hmms(0) == n
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(f, max_hmms=n - 1)
    assert str(e.value) == (f"ssw_grammar_prepare_large: grammar 0 (big) has {n} phone-tree HMMs: "
                            f"max_hmms allows at most {n - 1}")
    f = _loop_over_dictionary_words(m, lex, 200, 3400)
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(f, max_hmms=30000)
    got = re.fullmatch(r"ssw_grammar_prepare_large: grammar 0 \(big\) has (\d+) phone-tree HMMs: "
                       r"max_hmms allows at most 30000", str(e.value))
    assert got and int(got.group(1)) > 30000


def test_without_max_hmms_the_refusal_is_the_one_workgroup_one(host):
    _, lex, fsgs = host
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(fsgs["loop200"])
    assert str(e.value) == ("ssw_grammar_prepare: grammar 0 (loop200) has 5613 phone-tree HMMs: the "
                            "grammar search holds at most 4096 in one workgroup")


def test_history_groups_follow_the_budget(host, monkeypatch):
    """(frames + 1) x entering-list entries x 8 bytes per utterance: loop400 has 9826 entries,
    22,010,240 bytes at 279 frames.  On the large path a call is cut into groups that fit; a plan
    on the one-workgroup kernels is never cut (its call is refused as before)"""
    _, lex, fsgs = host
    plan = lex.grammar_plan([fsgs["loop200"], fsgs["loop400"]], max_hmms=30000)
    off = [0, 279, 558, 837]
    assert plan.history_groups(off, [1, 1, 1]) == 1
    assert plan.history_groups([0]) == 0
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "30")
    assert plan.history_groups(off, [1, 1, 1]) == 3
    assert plan.history_groups(off, [0, 0, 1]) == 2      # loop200: 4634 entries, 10.4 MB
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "20")
    with pytest.raises(ssw.SswError, match=r"utterance 2 .* exceeds the budget of 20971520 bytes"):
        plan.history_groups(off, [0, 0, 1])
    small = lex.grammar_plan(ssw.Fsg.read(host[0], lex, C.fsg_path("loop110")), max_hmms=30000)
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "1")
    with pytest.raises(ssw.SswError, match="exceeds the budget"):
        small.history_groups(off)


def test_ctypes_mirror_resolves_the_new_symbols():
    from soundswallower_amd import _lib
    L = _lib.lib()
    assert len(L.ssw_grammar_prepare_large.argtypes) == 6
    assert L.ssw_grammar_prepare_large.restype is not None
    assert len(L.ssw_grammar_history_groups.argtypes) == 4
    with open(_lib.HEADER, encoding="utf-8") as f:
        header = f.read()
    assert "#define SSW_GRAMMAR_LARGE_MAX_HMMS 30000" in header
