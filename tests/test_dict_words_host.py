"""Words added to a loaded dictionary (ssw_dict_add_word, ssw_dict_lookup_word; Lexicon.add_word,
Lexicon.lookup_word) on the host: no device needed.  The truth for return values, lookups and the
searched grammars is what the reference library printed for decoder_add_word,
decoder_lookup_word and fsg_model_write after decoder_set_fsg (tests/golden/inputs_words.json,
written by tests/golden/make_inputs.py).

Every test here needs the feature: Lexicon.add_word does not exist without it."""
import os

import pytest

import soundswallower_amd as ssw
from tests import inputs_common as I
from tests.conftest import MODEL_ROOT

RESULTS = I.word_results()


def _host(name):
    d = os.path.join(MODEL_ROOT, name)
    m = ssw.Model(d, config={"device": ssw.SSW_DEVICE_NONE})
    return m, ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))


def _add_all(lex, model):
    """the adds of inputs_common in order; the return values, -1 for a refusal"""
    out = []
    for w, p in I.adds(model):
        try:
            out.append([w, lex.add_word(w, p)])
        except (KeyError, ssw.SswError):
            out.append([w, -1])
    return out


@pytest.fixture(scope="module")
def grown():
    """model name -> (Model, Lexicon with the adds, their return values, size before)"""
    out = {}
    for name in ("en-us", "fr-fr"):
        m, lex = _host(name)
        n = len(lex)
        out[name] = (m, lex, _add_all(lex, name), n)
    return out


def _lines(text):
    assert text.endswith("\n")
    return text[:-1].split("\n")


def test_fixture_lists_the_cases():
    assert sorted(RESULTS) == sorted(I.word_key(c[0], comp) for c in I.WORD_CASES
                                     for comp in I.CONFIGS)


@pytest.mark.parametrize("model,case", [("en-us", "plain"), ("fr-fr", "fr")])
def test_return_values_and_lookups_are_the_references(grown, model, case):
    """ids are appended and equal the reference's: both load the same files in the same order"""
    m, lex, got, n0 = grown[model]
    fx = RESULTS[I.word_key(case, "yes")]
    assert got == fx["adds"]
    assert [[w, lex.lookup_word(w)] for w, _ in I.adds(model)] == fx["lookups"]
    ok = [rv for _, rv in got if rv >= 0]
    assert ok == list(range(n0, n0 + len(ok))) and len(lex) == n0 + len(ok)
    for w, rv in got:
        if rv >= 0:
            assert lex.word(rv) == w and lex.word_id(w) == rv


def test_refusals_leave_the_dictionary_unchanged():
    m, lex = _host("en-us")
    n = len(lex)
    with pytest.raises(KeyError):
        lex.add_word("forward", "F AO R W ER D")             # exists
    cases = [("qqnophone", "F XX", "Unknown phone XX in phone string F XX"),
             ("qqnobase(2)", "T EH N", "Missing base word for: qqnobase(2)"),
             ("qqempty", "", "no phones for 'qqempty'"),
             ("qqempty", " \t ", "no phones for 'qqempty'"),
             ("qqlong", " ".join(["AH"] * 257), "more than 256 phones for 'qqlong'"),
             ("qq word", "T EH N", "white space in the word 'qq word'"),
             ("", "T EH N", "bad arguments to ssw_dict_add_word")]
    for w, p, msg in cases:
        with pytest.raises(ssw.SswError) as e:
            lex.add_word(w, p)
        assert str(e.value) == "ssw_dict_add_word: " + msg
        assert len(lex) == n and lex.lookup_word(w) is None
    assert lex.add_word("qqlong", " ".join(["AH"] * 256)) == n    # what a dictionary line holds
    assert lex.lookup_word("qqlong") == " ".join(["AH"] * 256)
    with pytest.raises(KeyError):
        lex.add_word("qqlong", "AH")
    assert len(lex) == n + 1 and lex.lookup_word("nosuchword") is None


def test_lookup_round_trip(grown):
    for model in ("en-us", "fr-fr"):
        m, lex, _, _ = grown[model]
        for w, p in I.added(model):
            assert lex.lookup_word(w) == " ".join(p.split()) == " ".join(lex.pron(w))
    m, lex, _, _ = grown["en-us"]
    assert lex.lookup_word("forward") == "F AO R W ER D"
    # the C call: the length it needs, a cut and terminated copy in a short buffer
    import ctypes as C
    buf = C.create_string_buffer(b"x" * 8, 8)
    assert lex._L.ssw_dict_lookup_word(lex._d, m._m, b"forward", buf, 8) == 13
    assert buf.value == b"F AO R "
    assert lex._L.ssw_dict_lookup_word(lex._d, m._m, b"nosuchword", buf, 8) == -1


def test_filler_status(grown):
    for model in ("en-us", "fr-fr"):
        m, lex, got, n0 = grown[model]
        assert not any(lex.is_filler(rv) for _, rv in got if rv >= 0)
        assert lex.is_filler(lex.word_id("<sil>"))
        assert not lex.is_filler(lex.word_id("<s>")) and not lex.is_filler(lex.word_id("</s>"))
        assert [lex.is_filler(i) for i in range(n0)] == [lex.word(i).startswith(("<sil>", "[", "+"))
                                                         for i in range(n0)]
    m, lex, _, _ = grown["en-us"]
    assert lex.is_filler(lex.word_id("[NOISE]")) and lex.is_filler(lex.word_id("[SPEECH]"))


def _searched(m, lex, case):
    _, _, _, how, what = case
    if how == "fsg":
        name, n, start, final, trans = what
        f = ssw.Fsg.create(m, lex, name, start, final, list(trans), n_states=n)
    else:
        words = what.split()
        f = ssw.Fsg.create(m, lex, what, 0, len(words),
                           [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    return _lines(f.write(lex, searched=True))


@pytest.mark.parametrize("case", I.WORD_CASES, ids=[c[0] for c in I.WORD_CASES])
def test_searched_grammar_after_adds_is_the_references(grown, case):
    """an added word looped in as silence, or a filler word lost from the loops, shows here"""
    m, lex, _, _ = grown[case[1]]
    assert _searched(m, lex, case) == RESULTS[I.word_key(case[0], "yes")]["fsg_search"]
    assert RESULTS[I.word_key(case[0], "no")]["fsg_search"] == \
        RESULTS[I.word_key(case[0], "yes")]["fsg_search"]


@pytest.mark.parametrize("case", [c for c in I.WORD_CASES if c[3] == "text"],
                         ids=[c[0] for c in I.WORD_CASES if c[3] == "text"])
def test_text_graph_after_adds(grown, case):
    """first_pass_graph offers the words the reference's searched grammar offers: every
    alternate of the text's words, and as fillers exactly the words of its self loops"""
    m, lex, got, _ = grown[case[1]]
    nodes, _ = lex.first_pass_graph(case[4].split())
    mine = {lex.word(int(w)) for w in nodes["wid"] if w >= 0}
    want = {t.split(" ", 4)[4] for t in RESULTS[I.word_key(case[0], "yes")]["fsg_search"]
            if t.startswith("TRANSITION")}
    assert mine == want
    loops = {t.split(" ", 4)[4] for t in RESULTS[I.word_key(case[0], "yes")]["fsg_search"]
             if t.startswith("TRANSITION") and t.split()[1] == t.split()[2]}
    assert {w for w in mine if lex.is_filler(lex.word_id(w))} == loops
    assert not loops & {w for w, rv in got if rv >= 0}


def test_alternate_is_linked_at_the_head_and_snapshots_stay(grown):
    m, lex = _host("en-us")
    words = ["go", "forward"]
    before_nodes, _ = lex.first_pass_graph(words)
    f = ssw.Fsg.create(m, lex, "chain", 0, 2, [(0, 1, 1.0, "go"), (1, 2, 1.0, "forward")])
    before = f.write(lex, searched=True)
    plan = lex.grammar_plan(f)
    hmms = plan.hmms(0)
    p_go = lex._L.ssw_dict_word(lex._d, lex.word_id("go"))
    a = lex.add_word("forward(2)", "F AO R W ER D Z")
    b = lex.add_word("forward(3)", "F AO W ER D")
    after = _lines(f.write(lex, searched=True))
    # the word's list is walked newest first (forward -> (3) -> (2)) and fsg_model_add_alt
    # prepends each link it makes, so the state lists (2), (3), forward
    k = after.index("TRANSITION 1 2 1.000000 forward")
    assert after[k - 2:k] == ["TRANSITION 1 2 1.000000 forward(2)", "TRANSITION 1 2 1.000000 forward(3)"]
    assert len(after) == len(_lines(before)) + 2
    nodes, _ = lex.first_pass_graph(words)
    assert {a, b} <= {int(w) for w in nodes["wid"]} and len(nodes) > len(before_nodes)
    assert plan.hmms(0) == hmms                            # built before the add: a snapshot
    assert lex._L.ssw_dict_word(lex._d, lex.word_id("go")) == p_go


def test_growth_crosses_a_capacity_doubling_and_a_rehash(tmp_path):
    """a small dictionary starts at 4096 entries (and a hash table made for them): 5000 adds
    cross the doubling and its rehash; pointers handed out before stay valid"""
    d = os.path.join(MODEL_ROOT, "en-us")
    small = tmp_path / "small.dict"
    small.write_text("go G OW\nforward F AO R W ER D\n", encoding="utf-8")
    m = ssw.Model(d, config={"device": ssw.SSW_DEVICE_NONE})
    lex = ssw.Lexicon(m, str(small), os.path.join(d, "noisedict.txt"))
    n0 = len(lex)
    assert n0 < 4096
    early = lex._L.ssw_dict_word(lex._d, 0)
    ids = [lex.add_word(f"w{i}", "G OW" if i % 2 else "T EH N") for i in range(5000)]
    ids += [lex.add_word(f"w{i}(2)", "F AO R") for i in range(0, 5000, 1000)]
    assert ids == list(range(n0, n0 + 5005)) and len(lex) == n0 + 5005 > 4096
    assert all(lex.word_id(f"w{i}") == n0 + i for i in range(5000))
    assert all(lex.word(n0 + i) == f"w{i}" for i in range(0, 5000, 97))
    assert lex.lookup_word("w4999") == "G OW" and lex.lookup_word("w4000(2)") == "F AO R"
    assert lex.word_id("go") == 0 and lex._L.ssw_dict_word(lex._d, 0) == early == b"go"
    assert lex.is_filler(lex.word_id("[NOISE]")) and not lex.is_filler(n0 + 4999)
    lex.free()
