"""Word FSGs on the host (ssw_fsg_create, ssw_fsg_read, ssw_fsg_write, ssw_grammar_graph,
ssw_grammar_prepare): no device needed.  The truth is what the reference library wrote for the
same grammars (tests/golden/fsg_results.json: fsg_model_write after fsg_model_readfile, and again
after decoder_set_fsg)."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests.conftest import MODEL_ROOT

RESULTS = C.results()


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


def test_fixture_lists_the_seven_groups():
    assert sorted({v["group"] for v in RESULTS.values()}) == sorted(C.GROUPS)
    assert len(C.MANDATORY_GROUPS) == 7 and set(C.MANDATORY_GROUPS) <= set(C.GROUPS)
    assert sorted(RESULTS) == sorted(c[0] for c in C.CASES)
    for name, group, grammar, model, recording, samples in C.CASES:
        fx = RESULTS[name]
        assert (fx["group"], fx["grammar"], fx["model"], fx["recording"], fx["samples"]) == \
            (group, grammar, model, recording, samples)
        assert fx["json"].endswith("\n") and fx["frames"] > 0


@pytest.mark.parametrize("name", [c[0] for c in C.CASES if c[5] == 0])
def test_closure_and_link_order_as_the_reference_writes_them(host, name):
    """the null transitions closed with the best probability, every state's links in
    fsg_model_arcs order, before and after the search's silences and alternates"""
    fx = RESULTS[name]
    m, lex = host[fx["model"]]
    f = ssw.Fsg.read(m, lex, C.fsg_path(fx["grammar"]))
    assert _lines(f.write()) == fx["fsg"]
    assert _lines(f.write(lex, searched=True)) == fx["fsg_search"]


def test_nulls_closure_has_the_chain_and_the_best_probability(host):
    got = _lines(ssw.Fsg.read(*host["en-us"], C.fsg_path("nulls")).write())
    assert "TRANSITION 4 6 0.250066 " in got            # 4 -> 5 -> 6 closed: .5 x .5
    assert "TRANSITION 0 1 0.700065 " in got
    assert not [t for t in got if t.startswith("TRANSITION 7 7")]   # 7 -> 6 -> 7 needs a word


def test_read_and_create_give_the_same_grammar(host):
    m, lex = host["en-us"]
    a = ssw.Fsg.read(m, lex, C.fsg_path("nulls"))
    name, n, start, final, trans = C.parse_fsg(C.fsg_path("nulls"))
    b = ssw.Fsg.create(m, lex, name, start, final, trans, n_states=n)
    assert (a.name, a.n_states) == (b.name, b.n_states) == ("nulls", 9)
    assert a.write() == b.write()
    assert a.write(lex, searched=True) == b.write(lex, searched=True)
    na, ba = lex.grammar_graph(a)
    nb, bb = lex.grammar_graph(b)
    assert np.array_equal(na, nb) and np.array_equal(ba, bb)


def test_silences_and_alternates(host):
    """grammar 1 gets <sil> and [NOISE] loops on every state; grammar 4, which names <sil> and
    an alternate itself, is treated as the reference treats it: fsg_model_has_sil / _has_alt are
    false for a grammar that was read (only fsg_model_add_silence / _add_alt set them), so the
    loops are added and the grammar's own <sil> links keep their larger probability"""
    m, lex = host["en-us"]
    go = _lines(ssw.Fsg.read(m, lex, C.fsg_path("goforward")).write(lex, searched=True))
    for s in range(7):
        assert f"TRANSITION {s} {s} 0.005001 <sil>" in go
        assert f"TRANSITION {s} {s} 0.000000 [NOISE]" in go
    sil = _lines(ssw.Fsg.read(m, lex, C.fsg_path("sil")).write(lex, searched=True))
    assert sil == RESULTS["sil"]["fsg_search"]
    assert "TRANSITION 0 0 0.100010 <sil>" in sil and "TRANSITION 4 4 0.100010 <sil>" in sil
    assert "TRANSITION 1 1 0.005001 <sil>" in sil
    assert "TRANSITION 1 2 0.500091 hello(2)" in sil and not [t for t in sil if t.endswith(" hello")]
    # alternates go in front of the list that holds their word
    loop = _lines(ssw.Fsg.read(m, lex, C.fsg_path("loop")).write(lex, searched=True))
    assert loop[4] == "TRANSITION 0 0 0.125018 a(2)"
    # withheld on request
    f = ssw.Fsg.read(m, lex, C.fsg_path("loop"))
    bare = _lines(f.write(lex, cfg=lex.first_pass_config(use_filler=0, use_altpron=0), searched=True))
    assert bare == _lines(f.write())
    only_alt = _lines(f.write(lex, cfg=lex.first_pass_config(use_filler=0), searched=True))
    assert len(only_alt) == len(bare) + 1 and "TRANSITION 0 0 0.125018 a(2)" in only_alt


def _written(p, lw=6.5, base=1.0001):
    """what fsg_model_write prints for a probability: (int32)(logmath_log(p) * lw) going in
    (src/fsg_model.c:630), logmath_exp((int32)(logs2prob / lw)) coming out (:782-786), the
    products and quotients in float32"""
    logp = int(np.float32(int(np.log(np.float64(np.float32(p))) * (1.0 / np.log(base)))) * np.float32(lw))
    return "%f" % (base ** int(np.float32(logp) / np.float32(lw)))


def test_lw_scales_the_log_probabilities(host):
    m, lex = host["en-us"]
    assert (_written(0.5), _written(0.9), _written(0.1)) == ("0.500091", "0.900149", "0.100010")
    f = ssw.Fsg.read(m, lex, C.fsg_path("goforward"))
    for lw in (1.0, 9.5):
        a = _lines(f.write(lex, cfg=lex.first_pass_config(lw=lw)))
        assert "TRANSITION 5 6 %s meters" % _written(0.9, lw) in a
        assert "TRANSITION 4 5 %s ten" % _written(0.1, lw) in a


def _write(tmp_path, text):
    p = tmp_path / "g.fsg"
    p.write_text(text, encoding="utf-8")
    return str(p)


HEAD = "FSG_BEGIN g\nNUM_STATES 3\nSTART_STATE 0\nFINAL_STATE 2\n"


def test_reader_accepts_what_the_reference_accepts(host, tmp_path):
    m, lex = host["en-us"]
    text = ("# a comment\n\nFSG_BEGIN short\n# another\nN 3\nS 0\nF 2\n"
            "T 0 1 0.5 go\nTRANSITION 0 1 0.5 forward\n  T   1 2   1.0   \nsomething else\n"
            "T 1 2 0.25 ten\nFSG_END\nT 0 2 1.0 meters\n")
    f = ssw.Fsg.read(m, lex, _write(tmp_path, text))
    assert (f.name, f.n_states) == ("short", 3)
    assert _lines(f.write()) == ["FSG_BEGIN short", "NUM_STATES 3", "START_STATE 0",
                                 "FINAL_STATE 2", "TRANSITION 0 1 0.500091 forward",
                                 "TRANSITION 0 1 0.500091 go",
                                 "TRANSITION 1 2 %s ten" % _written(0.25),
                                 "TRANSITION 1 2 1.000000 ", "FSG_END"]
    # a link met again keeps the larger probability; a null self loop is dropped
    f = ssw.Fsg.read(m, lex, _write(tmp_path, HEAD + "T 0 1 0.1 go\nT 0 1 0.5 go\nT 1 1 0.5\n"
                                                     "T 1 2 0.5\nT 1 2 0.25\nFSG_END\n"))
    assert _lines(f.write())[4:-1] == ["TRANSITION 0 1 0.500091 go", "TRANSITION 1 2 0.500091 "]


@pytest.mark.parametrize("body,message", [
    ("NUM_STATES 3\n", "FSG_BEGIN declaration missing"),
    ("FSG_BEGIN g\nSTART_STATE 0\n", "NUM_STATES declaration missing"),
    ("FSG_BEGIN g\nNUM_STATES x\n", "NUM_STATES declaration malformed"),
    ("FSG_BEGIN g\nNUM_STATES 3\nFINAL_STATE 2\n", "START_STATE declaration missing"),
    ("FSG_BEGIN g\nNUM_STATES 3\nSTART_STATE 3\nFINAL_STATE 2\n", "START_STATE declaration malformed"),
    ("FSG_BEGIN g\nNUM_STATES 3\nSTART_STATE 0\n", "FINAL_STATE declaration missing"),
    ("FSG_BEGIN g\nNUM_STATES 3\nSTART_STATE 0\nFINAL_STATE -1\n", "FINAL_STATE declaration malformed"),
    (HEAD + "T\n", "Line[5]: from-state missing"),
    (HEAD + "T 3 1 0.5 go\n", "Invalid from-state 3"),
    (HEAD + "T 0\n", "Line[5]: to-state missing"),
    (HEAD + "T 0 -1 0.5 go\n", "Invalid to-state -1"),
    (HEAD + "T 0 1\n", "Line[5]: trans-prob missing"),
    (HEAD + "T 0 1 0.0 go\n", "Line[5]: transition spec malformed; Expecting float as transition probability"),
    (HEAD + "T 0 1 1.5 go\n", "Line[5]: transition spec malformed; Expecting float as transition probability"),
    (HEAD + "T 0 1 1.5\n", "Line[5]: transition spec malformed; Expecting float as transition probability"),
    (HEAD + "T 0 1 go\n", "Line[5]: transition spec malformed; Expecting float as transition probability"),
    (HEAD + "T 0 1 0.5 xyzzyplugh\nFSG_END\n", "The word 'xyzzyplugh' is missing in the dictionary"),
])
def test_reader_refusals(host, tmp_path, body, message):
    m, lex = host["en-us"]
    with pytest.raises(ssw.SswError) as e:
        ssw.Fsg.read(m, lex, _write(tmp_path, body))
    assert str(e.value) == "ssw_fsg_read: " + message


def test_unreadable_file(host, tmp_path):
    with pytest.raises(ssw.SswError, match="Failed to open FSG file"):
        ssw.Fsg.read(*host["en-us"], str(tmp_path / "none.fsg"))


@pytest.mark.parametrize("args,message", [
    ((0, 2, [(0, 3, 0.5, "go")], 3), "Invalid to-state 3"),
    ((0, 2, [(-1, 1, 0.5, "go")], 3), "Invalid from-state -1"),
    ((0, 2, [(0, 1, 0.0, "go")], 3), "Transition 0: transition spec malformed; Expecting float as transition probability"),
    ((0, 2, [(0, 1, 0.5, "go"), (1, 2, 1.25)], 3), "Transition 1: transition spec malformed; Expecting float as transition probability"),
    ((0, 2, [(0, 1, -0.5, "go")], 3), "Transition 0: transition spec malformed; Expecting float as transition probability"),
    ((3, 2, [(0, 1, 0.5, "go")], 3), "START_STATE declaration malformed"),
    ((0, 3, [(0, 1, 0.5, "go")], 3), "FINAL_STATE declaration malformed"),
    ((0, 2, [(0, 1, 0.5, "go"), (1, 2, 0.5, "xyzzyplugh")], 3), "The word 'xyzzyplugh' is missing in the dictionary"),
])
def test_create_refusals(host, args, message):
    m, lex = host["en-us"]
    start, final, trans, n = args
    with pytest.raises(ssw.SswError) as e:
        ssw.Fsg.create(m, lex, "g", start, final, trans, n_states=n)
    assert str(e.value) == "ssw_fsg_create: " + message


def test_unknown_word_is_refused_by_the_plan_when_create_had_no_dictionary(host):
    m, lex = host["en-us"]
    f = ssw.Fsg.create(m, None, "g", 0, 1, [(0, 1, 1.0, "xyzzyplugh")])
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(f)
    assert str(e.value) == "ssw_grammar_prepare: The word 'xyzzyplugh' is missing in the dictionary"


def test_grammar_over_the_hmm_limit_is_refused_by_the_plan(host):
    """(the refusal of a model with more than 64 CI phones cannot be shown: both models have
    fewer)"""
    m, lex = host["en-us"]
    words = [lex.word(i) for i in range(200, 3200)]
    words = [w for w in words if w and "(" not in w and not w.startswith("<")]
    f = ssw.Fsg.create(m, lex, "big", 0, 0, [(0, 0, 1.0 / len(words), w) for w in words])
    n = len(lex.grammar_graph(f)[0])
    assert n > 4096
    with pytest.raises(ssw.SswError) as e:
        lex.grammar_plan(f)
    assert str(e.value) == (f"ssw_grammar_prepare: grammar 0 (big) has {n} phone-tree HMMs: the "
                            "grammar search holds at most 4096 in one workgroup")


def test_plan_counts_the_hmms(host):
    m, lex = host["en-us"]
    fs = [ssw.Fsg.read(m, lex, C.fsg_path(g)) for g in ("goforward", "loop")]
    plan = lex.grammar_plan(fs)
    assert [plan.hmms(i) for i in range(2)] == [len(lex.grammar_graph(f)[0]) for f in fs]
    assert plan.hmms(2) == -1


@pytest.mark.parametrize("model,text", [
    ("en-us", "go forward ten meters"), ("en-us", "hello world"), ("en-us", "a"),
    ("en-us", "go go forward ten meters meters"), ("en-us", ""), ("fr-fr", "avance de dix mètres")])
def test_chain_grammar_graph_equals_the_text_graph(host, model, text):
    """the general builder on a chain FSG = the linear builder on the text, node for node: the
    same phone-tree HMMs with the same senones, penalties, predecessors, states, words, context
    sets and twin flags.  Only their numbering differs: the text's builder takes a state's links
    as word, alternates, <sil>, fillers, the grammar's in the reference's fsg_model_arcs order
    (the loops of a state before the links that leave it), so a node is compared by what it is and
    by what its chain of predecessors is, not by its index."""
    m, lex = host[model]
    words = text.split()
    want, wb = lex.first_pass_graph(words)
    f = ssw.Fsg.create(m, lex, "chain", 0, len(words),
                       [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    got, gb = lex.grammar_graph(f)
    assert np.array_equal(wb, gb)
    assert len(got) == len(want)

    def canon(nodes):
        def one(i):
            n = nodes[i]
            me = (tuple(int(x) for x in n["senid"]), int(n["tmat"]), int(n["pen"]),
                  int(n["flags"]), int(n["ci_ext"]), int(n["state"]), int(n["to_state"]),
                  int(n["wid"]), int(n["ctxt"]))
            return me + ((one(int(n["parent"])),) if n["parent"] >= 0 else ())
        return sorted(one(i) for i in range(len(nodes)))
    assert canon(got) == canon(want)
    # and within one link the order is the same: the nodes of any one word keep their sequence
    for w in {int(n["wid"]) for n in want if n["wid"] >= 0}:
        a = [tuple(int(x) for x in n["senid"]) for n in got if n["wid"] == w]
        b = [tuple(int(x) for x in n["senid"]) for n in want if n["wid"] == w]
        assert a == b


def test_contexts_cross_null_transitions(host):
    """fsg_lextree_lc_rc: the words that end at a state also end at the states a null leads to,
    and the words that leave those states also leave it"""
    m, lex = host["en-us"]
    nodes, _ = lex.grammar_graph(ssw.Fsg.read(m, lex, C.fsg_path("goforward")))
    ci = {p: i for i in range(64) for p in [lex._L.ssw_ciphone_name(m._m, i)] if p}
    # roots of state 4 (the numbers) must serve the last phone of "forward" / "backward" (D),
    # which end at states 2 and 3
    roots4 = [n for n in nodes if n["state"] == 4 and n["flags"] & 1 and not n["flags"] & 2]
    assert roots4 and all(int(n["ctxt"]) >> ci[b"D"] & 1 for n in roots4)
    # the word-final HMMs of "forward" (1 -> 2) must serve the first phones of the numbers
    fw = lex.word_id("forward")
    rc = 0
    for n in nodes:
        if n["wid"] == fw and n["flags"] & 2:
            rc |= int(n["ctxt"])
    for ph in (b"T", b"N", b"S", b"F", b"W", b"EY", b"TH"):   # ten two / nine / six seven / ...
        assert rc >> ci[ph] & 1, ph
