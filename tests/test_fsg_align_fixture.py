"""tests/golden/fsg_align_results.json (tests/golden/make_fsg_align.py): the reference's
decoder_result_json at align_level 1 and 2 and its decoder_alignment after a grammar, in both
configurations -- the fixture is whole, consistent with itself, and shows that the state the
first pass leaves behind is visible in the second pass's numbers."""
import json

import pytest

from tests import fsg_align_common as A

FRATE = 100


@pytest.fixture(scope="module")
def results():
    return A.results()


def test_every_case_is_recorded(results):
    assert sorted(results) == sorted(A.keys())
    for c in A.CASES:
        for cfg in A.configs(c):
            rec = results[c[0] + "/" + cfg]
            assert (rec["kind"], rec["grammar"], rec["model"], rec["recording"], rec["samples"],
                    rec["config"]) == (c[1], c[2], c[3], c[4], c[5], cfg)


def test_outcomes_seen_of_the_reference(results):
    for cfg in A.CONFIGS:
        for name in A.ALIGNED:
            rec = results[name + "/" + cfg]
            assert rec["hyp"] and rec["json1"] and rec["json2"] and rec["states"]
        for name in A.NO_HYP:
            rec = results[name + "/" + cfg]
            assert rec["hyp"] is None and rec["json1"] is None and rec["json2"] is None
            assert rec["words"] is None and rec["phones"] is None and rec["states"] is None
            # (a search that ended before any word exit logs nothing: the 410-sample cases)
            if rec["frames"] > 3:
                assert any("does not match the grammar" in e for e in rec["errors"])
    assert sum(1 for r in results.values() if r["json1"]) >= 2 * len(A.ALIGNED)


def _ticks(x):
    return round(x * FRATE)


def _tiles(parent, children):
    """children's (b, d) cover the parent's exactly, one after the other"""
    at = _ticks(parent["b"])
    for ch in children:
        assert _ticks(ch["b"]) == at
        at += _ticks(ch["d"])
    assert at == _ticks(parent["b"]) + _ticks(parent["d"])


@pytest.mark.parametrize("key", A.keys())
def test_lines_parse_and_nest(results, key):
    rec = results[key]
    l0 = json.loads(rec["json0"])
    assert rec["json0"].endswith("}\n") and l0["t"] == (rec["hyp"] or "")
    assert (rec["json1"] is None) == (rec["json2"] is None) == (rec["words"] is None)
    if rec["json1"] is None:
        assert rec["hyp"] is None and l0["w"] == []
        return
    l1, l2 = json.loads(rec["json1"]), json.loads(rec["json2"])
    for line in (l1, l2):
        assert (line["b"], line["d"], line["p"], line["t"]) == (l0["b"], l0["d"], l0["p"], l0["t"])
        assert line["d"] == pytest.approx(rec["frames"] / FRATE)
        # the word entries are the level-0 line's minus "(NULL)", same b and d
        want = [(w["t"], w["b"], w["d"]) for w in l0["w"] if w["t"] != "(NULL)"]
        assert [(w["t"], w["b"], w["d"]) for w in line["w"]] == want
        for w in line["w"]:
            assert w["w"]
            _tiles(w, w["w"])
    n_ph = n_st = 0
    for w1, w2 in zip(l1["w"], l2["w"]):
        assert [(p["t"], p["b"], p["d"], p["p"]) for p in w1["w"]] \
            == [(p["t"], p["b"], p["d"], p["p"]) for p in w2["w"]]
        for p1, p2 in zip(w1["w"], w2["w"]):
            assert "w" not in p1 and len(p2["w"]) == 3
            _tiles(p2, p2["w"])
            n_ph += 1
            n_st += len(p2["w"])
    # the entries of decoder_alignment are the same alignment in frames
    assert len(rec["words"]) == len(l1["w"]) and len(rec["phones"]) == n_ph
    assert len(rec["states"]) == n_st
    assert [(n, s, d) for n, s, d, _ in rec["words"]] \
        == [(w["t"], _ticks(w["b"]), _ticks(w["d"])) for w in l1["w"]]
    flat_ph = [p for w in l2["w"] for p in w["w"]]
    assert [(n, s, d) for n, s, d, _ in rec["phones"]] \
        == [(p["t"], _ticks(p["b"]), _ticks(p["d"])) for p in flat_ph]
    assert [(n, s, d) for n, s, d, _ in rec["states"]] \
        == [(s["t"], _ticks(s["b"]), _ticks(s["d"])) for p in flat_ph for s in p["w"]]
    # alignment_propagate: a parent's score is the sum of its children's
    assert sum(x[3] for x in rec["states"]) == sum(x[3] for x in rec["phones"]) \
        == sum(x[3] for x in rec["words"])


def test_the_seed_is_visible(results):
    """Under compallsen = no, loop400 and goforward recognise the same words (the first ones in
    the same frames), yet the scores of phones with the same window differ: the second pass starts
    from the senones the grammar search listed in its last frame.  A second pass that ignored the
    seed could not give both records."""
    a, b = results["goforward/no"], results["loop400/no"]
    assert [x[:3] for x in a["words"][:2]] == [x[:3] for x in b["words"][:2]]
    same = [(x, y) for x, y in zip(a["phones"], b["phones"]) if x[:3] == y[:3]]
    assert len(same) >= 10
    assert any(x[3] != y[3] for x, y in same)
    assert a["phones"][0][:3] == b["phones"][0][:3] == ["SIL", 0, 46]
    assert a["phones"][0][3] != b["phones"][0][3]
    # and the configuration is visible too
    y = results["goforward/yes"]
    assert [x[:3] for x in a["words"][:2]] == [x[:3] for x in y["words"][:2]]
    assert a["phones"][0][:3] == y["phones"][0][:3] and a["phones"][0][3] != y["phones"][0][3]
