"""Recognition against JSGF grammars on the GPU: Fsg.from_jsgf -> grammar_plan ->
recognize_audio_batch, in all four configurations of the grammar search (one workgroup and the
HBM-workspace kernel, compallsen = yes and the reference's default), against what the reference
library itself recognised through the steps of decoder_set_jsgf_file
(tests/golden/jsgf_results.json and jsgf_fsg_texts.json.gz, written by make_jsgf.py).  JSGF-born
grammars bring shapes no committed .fsg has: webs of weighted null transitions, a null entry at frame -1 in front of the
path, right-recursive loops.

Nothing is tolerated: status, message, words, frames, integer scores and the JSON line are compared
for equality."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from tests import jsgf_common as C
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

RESULTS = C.results()
SEARCHED = [c for c in C.CASES if RESULTS[c[0]]["refused"] is None
            and c[1] not in C.HOST_ONLY_GROUPS]
_cache = {}


def _lex(model, name):
    if ("lex", name) not in _cache:
        d = os.path.join(MODEL_ROOT, name)
        _cache["lex", name] = ssw.Lexicon(model, os.path.join(d, "dict.txt"),
                                          os.path.join(d, "noisedict.txt"))
    return _cache["lex", name]


def _fsg(model, case):
    _, _, grammar, name, _, _, toprule = case
    key = ("fsg", grammar, toprule)
    if key not in _cache:
        _cache[key] = ssw.Fsg.from_jsgf(model, _lex(model, name), path=C.gram_path(grammar),
                                        toprule=toprule)
    return _cache[key]


def _plan(model, cases, active):
    """one plan per list of grammars and kind, kept: its tables stay on the device"""
    large = any(c[2] in C.LARGE for c in cases)
    key = ("plan", tuple((c[2], c[6]) for c in cases), large, active and large)
    if key not in _cache:
        lex = _lex(model, cases[0][3])
        fsgs = [_fsg(model, c) for c in cases]
        _cache[key] = (lex.grammar_plan(fsgs, max_hmms=30000, active=active) if large
                       else lex.grammar_plan(fsgs))
    return _cache[key]


def _record(r, u):
    return {"status": r.status(u), "message": r.message(u), "hyp": r.hyp(u), "score": r.score(u),
            "segments": [list(s) for s in r.segments(u)], "json": r.json(u)}


def _expected(name, active):
    fx = RESULTS[name]["default" if active else "yes"]
    assert fx["hyp"] is not None
    return {"status": 0, "message": "", "hyp": fx["hyp"], "score": fx["score"],
            "segments": [s[:5] for s in fx["segments"]], "json": fx["json"]}


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
@pytest.mark.parametrize("name", [c[0] for c in SEARCHED])
def test_jsgf_case_as_the_reference_recognises_it(gpu_en, gpu_fr, name, active):
    """one recording per call; loop200 through grammar_plan(max_hmms=30000[, active=True])"""
    case = C.case(name)
    model = gpu_fr if case[3] == "fr-fr" else gpu_en
    pcm = C.pcm(case[4], case[5])
    plan = _plan(model, [case], active)
    if case[2] in C.LARGE:
        assert plan.hmms(0) > 4096
    r = ssw.recognize_audio_batch(model, _lex(model, case[3]), pcm, [0, len(pcm)], plan,
                                  active=active)
    got = _record(r, 0)
    print(name, plan.hmms(0), "HMMs", got)
    assert got == _expected(name, active)


def test_the_null_entry_at_frame_minus_one_is_reported(gpu_en):
    case = C.case("turtle")
    pcm = C.pcm(case[4], 0)
    r = ssw.recognize_audio_batch(gpu_en, _lex(gpu_en, "en-us"), pcm, [0, len(pcm)],
                                  _plan(gpu_en, [case], False))
    first = r.segments(0)[0]
    assert first[:3] == ("(NULL)", -1, -1) and list(first) == RESULTS["turtle"]["yes"]["segments"][0][:5]


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
def test_all_en_us_cases_as_one_batch_with_their_own_grammars(gpu_en, active):
    """per-utterance grammars, the cut recording among them: what each gave alone"""
    cases = [c for c in SEARCHED if c[3] == "en-us" and c[2] not in C.LARGE]
    assert any(c[5] for c in cases) and len(cases) >= 7
    grammars = []
    for c in cases:
        if (c[2], c[6]) not in grammars:
            grammars.append((c[2], c[6]))
    plan_cases = [next(c for c in cases if (c[2], c[6]) == g) for g in grammars]
    plan = _plan(gpu_en, plan_cases, active)
    pcms = [C.pcm(c[4], c[5]) for c in cases]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])])
    which = [grammars.index((c[2], c[6])) for c in cases]
    lex = _lex(gpu_en, "en-us")
    r = ssw.recognize_audio_batch(gpu_en, lex, np.concatenate(pcms), off, plan, which,
                                  active=active)
    for u, c in enumerate(cases):
        assert _record(r, u) == _expected(c[0], active), c[0]
        alone = ssw.recognize_audio_batch(gpu_en, lex, pcms[u], [0, len(pcms[u])],
                                          _plan(gpu_en, [c], active), active=active)
        assert _record(alone, 0) == _record(r, u), c[0]


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
def test_small_jsgf_grammars_beside_loop200_on_the_large_kernel(gpu_en, active):
    """one grammar beyond one workgroup puts the whole plan on the HBM-workspace kernel: the null
    entry, the closures and the weights give their records there too"""
    names = ("loop200", "turtle", "kleene", "weights", "recursion", "turtle_1200ms")
    cases = [C.case(n) for n in names]
    plan = _plan(gpu_en, cases[:5], active)
    pcms = [C.pcm(c[4], c[5]) for c in cases]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])])
    r = ssw.recognize_audio_batch(gpu_en, _lex(gpu_en, "en-us"), np.concatenate(pcms), off, plan,
                                  [0, 1, 2, 3, 4, 1], active=active)
    for u, n in enumerate(names):
        assert _record(r, u) == _expected(n, active), n
