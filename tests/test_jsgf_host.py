"""JSGF grammars on the host (ssw_jsgf_parse_*, ssw_jsgf_build_fsg, ssw_fsg_from_jsgf_*): no device
needed.  The truth is what the reference library itself made of the grammars under
tests/golden/jsgf/ (tests/golden/jsgf_results.json and jsgf_fsg_texts.json.gz, written by
make_jsgf.py): the rule table in jsgf_rule_iter order, the rule decoder_set_jsgf_* picks, fsg_model_write after jsgf_build_fsg, after
a second jsgf_build_fsg of the same parsed grammar, and after decoder_set_fsg."""
import os
import re

import pytest

import soundswallower_amd as ssw
from tests import jsgf_common as C
from tests.conftest import MODEL_ROOT

RESULTS = C.results()
HEADER_H = os.path.join(os.path.dirname(MODEL_ROOT), os.pardir, "include", "ssw_amd.h")


@pytest.fixture(scope="module")
def host():
    """model without a device + lexicon, per model name"""
    out = {}
    for name in ("en-us", "fr-fr"):
        d = os.path.join(MODEL_ROOT, name)
        m = ssw.Model(d, config={"device": -2})
        out[name] = (m, ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt")))
    return out


def _lines(text):
    assert text.endswith("\n")
    return text[:-1].split("\n")


def _text(grammar):
    with open(C.gram_path(grammar), encoding="utf-8") as f:
        return f.read()


def _rule(j, toprule):
    return j.public_rule() if toprule is None else j.find_rule(toprule)


def test_fixture_lists_the_cases():
    assert sorted(RESULTS) == sorted(c[0] for c in C.CASES)
    assert sorted({v["group"] for v in RESULTS.values()}) == sorted(C.GROUPS)
    for name, group, grammar, model, recording, samples, toprule in C.CASES:
        fx = RESULTS[name]
        assert (fx["group"], fx["grammar"], fx["model"], fx["recording"], fx["samples"],
                fx["toprule"]) == (group, grammar, model, recording, samples, toprule)
        for config in C.CONFIGS:
            if fx["refused"] is None:
                assert fx[config]["json"].endswith("\n") and fx[config]["frames"] > 0
                assert fx[config]["hyp"], name          # the reference recognises every case
    assert _text("loop200") == C.loop200_text()


def test_the_shapes_the_issue_is_about_are_in_the_fixture():
    """a null entry at frame -1 in front of the path, weighted nulls, a second build that differs"""
    assert RESULTS["turtle"]["yes"]["segments"][0][:3] == ["(NULL)", -1, -1]
    assert RESULTS["turtle"]["chosen"] == "<turtle.order>"
    assert RESULTS["turtle_halt"]["yes"]["hyp"] == "stop please"
    assert RESULTS["fr"]["yes"]["hyp"] == "avance de dix mètres"
    assert [s[0] for s in RESULTS["fr"]["yes"]["segments"] if s[0].startswith(("de", "mè"))] \
        == ["de(2)", "mètres(4)"]
    assert [s[4] for s in RESULTS["weights"]["yes"]["segments"]][1:6:2] == [-3, -14, -7]
    assert RESULTS["weights"]["fsg"] != RESULTS["weights"]["fsg_second"]
    assert RESULTS["weights"]["yes"]["score"] != RESULTS["weights"]["default"]["score"]


@pytest.mark.parametrize("name", [c[0] for c in C.CASES])
def test_rule_table_and_chosen_rule_as_the_reference_lists_them(name):
    _, _, grammar, _, _, _, toprule = C.case(name)
    fx = RESULTS[name]
    j = ssw.Jsgf.parse_file(C.gram_path(grammar))
    assert j.name == fx["name"]
    assert [list(r) for r in j.rules()] == fx["rules"]
    i = _rule(j, toprule)
    if fx["chosen"] is None:
        assert i is None and fx["refused"] == "Start rule %s not found" % toprule
    else:
        assert j.rules()[i][0] == fx["chosen"]
    # string and file parsing agree
    js = ssw.Jsgf.parse_string(_text(grammar))
    assert (js.name, js.rules(), _rule(js, toprule)) == (j.name, j.rules(), i)


@pytest.mark.parametrize("name", [c[0] for c in C.CASES if RESULTS[c[0]]["chosen"]])
def test_expansion_closure_and_link_order_as_the_reference_writes_them(host, name):
    """state numbers, link order and probabilities of jsgf_build_fsg; the second build from the
    same parsed grammar starts from the weights the first one left; and after decoder_set_fsg"""
    _, _, grammar, model, _, _, toprule = C.case(name)
    fx = RESULTS[name]
    m, lex = host[model]
    j = ssw.Jsgf.parse_file(C.gram_path(grammar))
    i = _rule(j, toprule)
    f = j.fsg(m, None, i)
    assert f.name == fx["chosen"] == fx["fsg"][0].split(" ", 1)[1]
    assert _lines(f.write()) == fx["fsg"]
    f2 = j.fsg(m, None, i)
    assert _lines(f2.write()) == fx["fsg_second"]
    assert _lines(f.write()) == fx["fsg"]                    # the first is its own
    # the one-call entry points, from the text and from the file: a fresh parse each
    by_text = (lambda lx: ssw.Fsg.from_jsgf(m, lx, text=_text(grammar), toprule=toprule))
    by_path = (lambda lx: ssw.Fsg.from_jsgf(m, lx, path=C.gram_path(grammar), toprule=toprule))
    if fx["refused"] is None:
        assert _lines(f.write(lex, searched=True)) == fx["fsg_search"]
        for g in (by_text(lex), by_path(lex), by_text(None)):
            assert _lines(g.write()) == fx["fsg"]
            assert _lines(g.write(lex, searched=True)) == fx["fsg_search"]
    else:
        assert fx["refused"] == "decoder_set_fsg"
        for make in (by_text, by_path):
            with pytest.raises(ssw.SswError) as e:
                make(lex)
            assert str(e.value).endswith(fx["yes"]["errors"][-1])
        assert _lines(by_text(None).write()) == fx["fsg"]     # (unchecked without a dictionary)


def test_the_quoted_word_keeps_its_quotes_and_is_missing(host):
    m, lex = host["en-us"]
    with pytest.raises(ssw.SswError, match=re.escape("The word '\"nine\"' is missing in the dictionary")):
        ssw.Fsg.from_jsgf(m, lex, path=C.gram_path("tags_quoted"))
    assert RESULTS["tags_quoted"]["yes"]["errors"] == ["The word '\"nine\"' is missing in the dictionary"]


def test_toprule_is_looked_up_verbatim(host):
    m, lex = host["en-us"]
    f = ssw.Fsg.from_jsgf(m, lex, text=_text("turtle"), toprule="turtle.halt")
    assert (f.name, f.n_states) == ("<turtle.halt>", 7)
    for make in (lambda: ssw.Fsg.from_jsgf(m, lex, text=_text("turtle"), toprule="halt"),
                 lambda: ssw.Fsg.from_jsgf(m, lex, path=C.gram_path("turtle"), toprule="halt")):
        with pytest.raises(ssw.SswError, match="Start rule halt not found"):
            make()
    assert RESULTS["turtle_unqualified"]["refused"] == "Start rule halt not found"
    j = ssw.Jsgf.parse_string(_text("turtle"))
    assert j.find_rule("halt") is None and j.find_rule("turtle.halt") is not None
    with pytest.raises(ssw.SswError, match="Start rule halt not found"):
        j.fsg(m, lex, "halt")


HEAD = "#JSGF V1.0;\ngrammar t;\n"


@pytest.mark.parametrize("text,line", [
    (HEAD + "public <a> = go\n  | ;\n", 4),                 # an empty alternative
    (HEAD + "public <a> = ;\n", 3),                         # an empty rule
    (HEAD + "public <a> = go );\n", 3),                     # a stray )
    (HEAD + "public <a> = ( go ;\n", 3),
    (HEAD + "public <a> = go {unterminated ;\n", 3),
    (HEAD + "public <a> = go /0.5 ten;\n", 3),              # an unterminated weight
    (HEAD + "public <a> = go /1e5/ ten;\n", 3),             # not the scanner's number format
    (HEAD + "public <a> = go\n /* never closed ;\n", 5),   # the comment runs to the end
    (HEAD + "public <a> = go {tag} * ;\n", 3),              # * after a tag
    (HEAD + "public <a> = go\n\n", 5),                      # the input ends inside the rule
    ("grammar t;\npublic <a> = go;\n", 1),                  # no #JSGF header
    ("#JSGF V1.0 UTF-8 en extra;\ngrammar t;\n", 1),        # a fourth header token
    ("", 1),
])
def test_syntax_errors_name_the_line(text, line):
    """the line the offending token ends on, counted from 1 (the reference's counter, which starts
    at 0 for a string, gives one less for every one of these)"""
    with pytest.raises(ssw.SswError) as e:
        ssw.Jsgf.parse_string(text)
    assert "syntax error" in str(e.value) and ("at line %d" % line) in str(e.value), str(e.value)


def test_what_the_scanner_accepts(host):
    m, lex = host["en-us"]
    # BOM, 0 to 3 header tokens, comments between and inside declarations, a comment that never
    # closes after the last rule, stuff between declarations
    for head in ("#JSGF;", "\ufeff#JSGF V1.0;", "#JSGF V1.0 UTF-8;", "#JSGF V1.0 UTF-8 en;"):
        j = ssw.Jsgf.parse_string(head + " // x\ngrammar g; /* y */ stray words\n"
                                  "public <a> = go // why\n /* and */ forward; /* open")
        assert j.name == "g" and j.rules() == [("<g.a>", True)]
        assert _lines(j.fsg(m, lex).write())[1:4] == ["NUM_STATES 4", "START_STATE 0", "FINAL_STATE 1"]
    # a name defined twice keeps its first definition; the group of the second is still numbered
    j = ssw.Jsgf.parse_string(HEAD + "public <a> = go; <a> = (stop); public <b> = [ten];")
    assert sorted(j.rules()) == [("<t.a>", True), ("<t.b>", True), ("<t.g00001>", False),
                                 ("<t.g00002>", False)]
    assert " go" in j.fsg(m, lex, "t.a").write()
    # a tag ends at the last brace that every brace before it is escaped for (the scanner's longest
    # match): the second text's tag swallows "forward"; "//" at the very end is a weight of 0
    def words(text):
        f = ssw.Fsg.from_jsgf(m, None, text=HEAD + text)
        return [t.split(" ", 4)[4] for t in _lines(f.write())
                if t.startswith("TRANSITION") and t.split(" ", 4)[4]]
    assert words(r"public <a> = go {a \} b} forward {c\\};") == ["go", "forward"]
    assert words(r"public <a> = go {a \} b} {c\\} forward {};") == ["go"]
    assert words('public <a> = "go forward" ten;') == ['"go forward"', "ten"]
    with pytest.raises(ssw.SswError, match=r"Rule <t\.a>: the weight of go is 0 "):
        ssw.Fsg.from_jsgf(m, lex, text=HEAD + "public <a> = // go | stop ;")


def test_refusals(host, tmp_path):
    m, lex = host["en-us"]

    def refused(text, message, **kw):
        with pytest.raises(ssw.SswError) as e:
            ssw.Fsg.from_jsgf(m, lex, text=text, **kw)
        assert message in str(e.value), str(e.value)

    # no public rule, from a string and from a file
    refused(HEAD + "<a> = go;", "No public rules found in input string")
    p = tmp_path / "private.gram"
    p.write_text(HEAD + "<a> = go;")
    with pytest.raises(ssw.SswError) as e:
        ssw.Fsg.from_jsgf(m, lex, path=str(p))
    assert ("No public rules found in %s" % p) in str(e.value)
    with pytest.raises(ssw.SswError, match="Failed to open .*nowhere.gram for parsing"):
        ssw.Fsg.from_jsgf(m, lex, path=str(tmp_path / "nowhere.gram"))
    refused(HEAD + "public <a> = go;", "Start rule t.b not found", toprule="t.b")
    refused(HEAD + "public <a> = go zzzyzzy;", "The word 'zzzyzzy' is missing in the dictionary")
    # weights that are not in (0, 1] after normalisation: only the leading one is normalised
    refused(HEAD + "public <a> = go /3/ forward;", "Rule <t.a>: the weight of forward is 3 ")
    refused(HEAD + "public <a> = /0/ go | stop;", "Rule <t.a>: the weight of go is 0 ")
    refused(HEAD + "public <a> = <b> ten; <b> = go /1.5/ <c>; <c> = stop;",
            "Rule <t.b>: the weight of <c> is 1.5 ")
    # imports
    refused("#JSGF V1.0;\ngrammar t;\nimport <other.rule>;\npublic <a> = go;",
            "import at line 3: imported grammars are not supported")
    # the three half-grammars the reference goes on to search
    refused(HEAD + "public <t> = go <where> ten meters;", "Undefined rule in RHS: <t.where>")
    refused(HEAD + "public <a> = go <a> stop | ten;",
            "Only right-recursion is permitted (in t.<t.a>)")
    refused(HEAD + "public <a> = go <b>; <b> = <a> stop | ten;",
            "Only right-recursion is permitted (in t.<t.b>)")
    refused(HEAD + "public <a> = go | <VOID> stop;", "<VOID> in <t.a>")


def test_the_header_says_what_is_deliberately_different():
    with open(HEADER_H, encoding="utf-8") as f:
        text = " ".join(f.read().split())
    assert "a deliberate difference" in text and "Undefined rule in RHS" in text


def test_loop200_is_beyond_one_workgroup(host):
    m, lex = host["en-us"]
    f = ssw.Fsg.from_jsgf(m, lex, path=C.gram_path("loop200"))
    assert f.n_states == int(RESULTS["loop200"]["fsg"][1].split()[1])
    plan = lex.grammar_plan(f, max_hmms=30000)
    max_hmms = int(re.search(r"#define SSW_GRAMMAR_MAX_HMMS (\d+)", open(HEADER_H).read()).group(1))
    assert plan.hmms(0) > max_hmms
    assert lex.grammar_plan(f, max_hmms=30000, active=True).hmms(0) == plan.hmms(0)
    with pytest.raises(ssw.SswError, match=str(plan.hmms(0))):
        lex.grammar_plan(f)
