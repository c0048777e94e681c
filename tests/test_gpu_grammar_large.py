"""Recognition against grammars of more than 4096 phone-tree HMMs on the GPU
(ssw_grammar_prepare_large -> grammar_search_big_kernel) against what the reference library
itself recognised (tests/golden/fsg_large_results.json, written by make_fsg_large.py), and the
committed small-grammar truths (fsg_results.json) searched by the same kernel.

Nothing is tolerated: words, frames, integer scores and the JSON line are compared for
equality."""
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests import fsg_large_common as CL
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

RESULTS = dict(C.results(), **CL.results())
_cache = {}


def _lex(model):
    if "lex" not in _cache:
        d = os.path.join(MODEL_ROOT, "en-us")
        _cache["lex"] = ssw.Lexicon(model, os.path.join(d, "dict.txt"),
                                    os.path.join(d, "noisedict.txt"))
    return _cache["lex"]


def _scores(model, samples):
    """senone scores (compallsen = yes) of the first `samples` samples of goforward.raw, once per
    session"""
    key = ("scr", samples)
    if key not in _cache:
        cep, _ = model.fe_batch(C.pcm("goforward.raw", samples))
        _cache[key] = model.score_batch(model.feat_batch(cep))
    return _cache[key]


def _fsg(model, grammar):
    key = ("fsg", grammar)
    if key not in _cache:
        _cache[key] = ssw.Fsg.read(model, _lex(model), C.fsg_path(grammar))
    return _cache[key]


def _plan(model, grammars, max_hmms=30000):
    """one plan per list of grammars, kept: its tables stay on the device between tests"""
    key = ("plan", tuple(grammars), max_hmms)
    if key not in _cache:
        _cache[key] = _lex(model).grammar_plan([_fsg(model, g) for g in grammars],
                                               max_hmms=max_hmms)
    return _cache[key]


def _search(model, scr_list, plan, fsg_of_utt=None):
    off = np.concatenate([[0], np.cumsum([len(s) for s in scr_list])]).astype(np.int32)
    d = torch.from_numpy(np.ascontiguousarray(np.concatenate(scr_list), np.int16)).cuda()
    return ssw.grammar_search_batch(model, _lex(model), d, off, plan, fsg_of_utt)


def _record(r, u):
    """utterance u of a RecognitionSet in the fixture's terms"""
    return {"status": r.status(u), "message": r.message(u), "hyp": r.hyp(u), "score": r.score(u),
            "segments": [list(s) for s in r.segments(u)], "json": r.json(u)}


def _expected(name):
    fx = RESULTS[name]
    if fx["hyp"] is not None:
        status, message = 0, ""
    elif fx["errors"]:
        status, message = 1, fx["errors"][-1]
    else:
        status, message = 2, "No hypothesis: no word exit in any frame"
    return {"status": status, "message": message, "hyp": fx["hyp"], "score": fx["score"],
            "segments": [s[:5] for s in fx["segments"]], "json": fx["json"]}


@pytest.mark.parametrize("name", [c[0] for c in CL.CASES])
def test_large_fixture_case(gpu_en, name):
    """every case the reference recorded, one utterance per call"""
    _, _, grammar, _, _, samples = next(c for c in CL.CASES if c[0] == name)
    scr = _scores(gpu_en, samples)
    assert len(scr) + 1 == RESULTS[name]["frames"]      # decoder_n_frames counts one more
    plan = _plan(gpu_en, [grammar])
    assert plan.hmms(0) == CL.HMMS[grammar]
    got = _record(_search(gpu_en, [scr], plan), 0)
    print(name, got)
    assert got == _expected(name)


def test_the_small_truths_on_the_large_kernel(gpu_en):
    """one grammar beyond the one-workgroup limits puts the whole plan on the HBM-workspace
    kernel: start-state nulls, no match, silence, twins and truncations give their committed
    records there, and loop200 beside them its own"""
    grammars = ["loop200", "goforward", "nulls", "loop", "sil", "nomatch"]
    plan = _plan(gpu_en, grammars)
    cases = [("loop200", "loop200", 0)] + [(g, g, 0) for g in grammars[1:]]
    cases += [(c[0], c[2], c[5]) for c in C.CASES if c[0] in ("goforward_410", "loop_410")]
    assert len(cases) == 8
    r = _search(gpu_en, [_scores(gpu_en, s) for _, _, s in cases], plan,
                [grammars.index(g) for _, g, _ in cases])
    for u, (name, _, _) in enumerate(cases):
        assert _record(r, u) == _expected(name), name


def test_two_large_grammars_alternating_and_the_call_repeated(gpu_en):
    """per-utterance workspace and history offsets; the second call finds the tables on the
    device"""
    plan = _plan(gpu_en, ["loop200", "loop400"])
    scr = _scores(gpu_en, 0)
    which = [0, 1] * 4
    r = _search(gpu_en, [scr] * 8, plan, which)
    for u, g in enumerate(which):
        assert _record(r, u) == _expected(("loop200", "loop400")[g]), u
    r2 = _search(gpu_en, [scr] * 8, plan, which)
    assert [_record(r2, u) for u in range(8)] == [_record(r, u) for u in range(8)]


def test_a_call_beyond_the_history_budget_is_searched_in_groups(gpu_en, monkeypatch):
    """loop400's history is 280 rows x 9826 entries x 8 bytes = 22.0 MB per utterance: under a
    30 MB budget three of them are three launches, under 20 MB one alone is refused"""
    plan = _plan(gpu_en, ["loop400"])
    scr = _scores(gpu_en, 0)
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "30")
    assert plan.history_groups([0, 279, 558, 837]) == 3
    r = _search(gpu_en, [scr] * 3, plan)
    for u in range(3):
        assert _record(r, u) == _expected("loop400"), u
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "20")
    with pytest.raises(ssw.SswError, match="exceeds the budget"):
        _search(gpu_en, [scr] * 3, plan)


def test_small_grammars_through_the_new_entry_point(gpu_en):
    """a plan made with max_hmms whose grammars all fit one workgroup: the existing kernels"""
    plan = _plan(gpu_en, ["goforward", "loop110"])
    scr = _scores(gpu_en, 0)
    assert plan.history_groups([0, 279, 558]) == 1
    r = _search(gpu_en, [scr] * 2, plan, [0, 1])
    assert _record(r, 0) == _expected("goforward")
    assert _record(r, 1) == _expected("loop110")


def test_recognize_audio_batch_on_a_large_grammar(gpu_en):
    """PCM in, the reference's JSON line out"""
    pcm = C.pcm("goforward.raw", 0)
    plan = _plan(gpu_en, ["loop200"])
    r = ssw.recognize_audio_batch(gpu_en, _lex(gpu_en), pcm, [0, len(pcm)], plan)
    assert r.json(0) == RESULTS["loop200"]["json"]
    assert r.hyp(0) == RESULTS["loop200"]["hyp"] and r.score(0) == RESULTS["loop200"]["score"]


def test_the_default_configuration_refuses_a_large_plan(gpu_en):
    pcm = C.pcm("goforward.raw", 0)
    plan = _plan(gpu_en, ["loop200"])
    with pytest.raises(ssw.SswError, match=r"grammar 0 \(loop200\) has 5613 phone-tree HMMs"):
        ssw.recognize_audio_batch(gpu_en, _lex(gpu_en), pcm, [0, len(pcm)], plan, active=True)
