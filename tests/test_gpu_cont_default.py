"""The reference's own numbers for continuous models in its DEFAULT configuration (compallsen =
no): tests/golden/cont_default_results.json, recorded by tests/golden/make_cont_default.py from
the reference library with the models C3 and C1, against the *_active entry points on models
with enable_active: recognition against goforward, loop, nulls, loop400 (a large active plan) and
jsgf/turtle.gram, the alignment of "go forward ten meters" at align levels 0, 1 and 2, and
goforward recognised and then aligned.  Equal in every field; where the reference has no
hypothesis, that status and message are the result."""
import json
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import cont_common as CC

pytestmark = pytest.mark.gpu

RESULTS_JSON = os.path.join(CC.GOLD, "cont_default_results.json")
FSGS = ("goforward", "loop", "nulls", "loop400")
TEXT = "go forward ten meters"
NO_EXIT = "No hypothesis: no word exit in any frame"


@pytest.fixture(scope="module")
def fx():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)


@pytest.fixture(scope="module")
def pcm():
    return np.fromfile(os.path.join(CC.GOLD, "goforward.raw"), dtype="<i2")


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("cont_default_gpu"))
    out = {}
    for name in ("C3", "C1"):
        d = CC.BUILDERS[name](os.path.join(tmp, name))
        m = ssw.Model(**CC.model_paths(d), active=True)
        assert m.continuous and m.active_enabled
        out[name] = (m, ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt")))
    return out


def _expected(rec):
    if rec["hyp"] is not None:
        status, message = 0, ""
    elif rec["errors"]:
        status, message = 1, rec["errors"][-1]
    else:
        status, message = 2, NO_EXIT
    return {"status": status, "message": message, "hyp": rec["hyp"], "score": rec["score"],
            "segments": [s[:5] for s in rec["segments"]], "json": rec["json"]}


def _record(r, u):
    return {"status": r.status(u), "message": r.message(u), "hyp": r.hyp(u), "score": r.score(u),
            "segments": [list(s) for s in r.segments(u)], "json": r.json(u)}


def _plan(model, lex, grammar):
    if grammar == "turtle":
        fsg = ssw.Fsg.from_jsgf(model, lex, path=os.path.join(CC.GOLD, "jsgf", "turtle.gram"))
    else:
        fsg = ssw.Fsg.read(model, lex, os.path.join(CC.GOLD, "fsg", grammar + ".fsg"))
    if grammar == "loop400":   # beyond one workgroup: the large plan of the default configuration
        plan = lex.grammar_plan([fsg], max_hmms=30000, active=True)
        assert plan.active
        return plan
    return lex.grammar_plan(fsg)


@pytest.mark.parametrize("grammar", FSGS + ("turtle",))
@pytest.mark.parametrize("name", ["C3", "C1"])
def test_recognition(models, fx, pcm, name, grammar):
    model, lex = models[name]
    rec = fx[name]["rec"][grammar]
    r = ssw.recognize_audio_batch(model, lex, pcm, [0, len(pcm)], _plan(model, lex, grammar), active=True)
    try:
        got = _record(r, 0)
        print(name, grammar, got["status"], got["hyp"], got["score"])
        assert got == _expected(rec)
    finally:
        r.free()


@pytest.mark.parametrize("name", ["C3", "C1"])
def test_text_alignment_at_every_level(models, fx, pcm, name):
    model, lex = models[name]
    rec = fx[name]["align"]
    a = ssw.align_audio_batch(model, lex, pcm, [0, len(pcm)], [TEXT.split()], active=True)
    try:
        if rec["json1"] is None:
            assert a.status(0) != 0
            assert rec["errors"] and a.message(0) == rec["errors"][-1]
            return
        assert a.status(0) == 0, a.message(0)
        for level in (1, 2):
            assert a.json(0, align_level=level).rstrip("\n") == rec["json%d" % level].rstrip("\n"), level
    finally:
        a.free()
    # align level 0 is the first pass's own hypothesis (ssw_alignment_set_json starts at level 1):
    # decoder_set_align_text searches the chain grammar of the words, every transition at
    # probability 1 (src/decoder.c:686-737), and so does this
    words = TEXT.split()
    chain = ssw.Fsg.create(model, lex, TEXT, 0, len(words), [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    r = ssw.recognize_audio_batch(model, lex, pcm, [0, len(pcm)], lex.grammar_plan(chain), active=True)
    try:
        assert r.status(0) == 0, r.message(0)
        assert r.json(0) == rec["json0"]
    finally:
        r.free()


@pytest.mark.parametrize("name", ["C3", "C1"])
def test_recognise_then_align(models, fx, pcm, name):
    model, lex = models[name]
    rec = fx[name]["rec_align"]
    r, a = ssw.recognize_align_audio_batch(model, lex, pcm, [0, len(pcm)],
                                           _plan(model, lex, "goforward"), active=True)
    try:
        assert (r.hyp(0), r.score(0), r.json(0)) == (rec["hyp"], rec["score"], rec["json0"])
        if rec["json1"] is None:
            assert a.status(0) != 0
            return
        assert a.status(0) == 0, a.message(0)
        assert a.json(0, align_level=1).rstrip("\n") == rec["json1"].rstrip("\n")
        assert a.json(0, align_level=2).rstrip("\n") == rec["json2"].rstrip("\n")
    finally:
        r.free()
        a.free()
