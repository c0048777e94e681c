"""Recognition against word FSGs on the GPU (ssw_grammar_search_batch, ssw_recognize_batch)
against what the reference library itself recognised (tests/golden/fsg_results.json, written by
tests/golden/make_fsg.py) and against the first pass of forced alignment on chain grammars.

Nothing is tolerated: words, frames, integer scores and the JSON line are compared for
equality."""
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

RESULTS = C.results()
_cache = {}


def _lex(model, name):
    key = ("lex", name)
    if key not in _cache:
        d = os.path.join(MODEL_ROOT, name)
        _cache[key] = ssw.Lexicon(model, os.path.join(d, "dict.txt"),
                                  os.path.join(d, "noisedict.txt"))
    return _cache[key]


def _scores(model, name, recording, samples):
    """senone scores (compallsen = yes) of the first `samples` samples of a recording: front end,
    dynamic features and scoring on the GPU, once per session"""
    key = ("scr", name, recording, samples)
    if key not in _cache:
        cep, _ = model.fe_batch(C.pcm(recording, samples))
        _cache[key] = model.score_batch(model.feat_batch(cep))
    return _cache[key]


def _fsg(model, lex, name, grammar):
    key = ("fsg", name, grammar)
    if key not in _cache:
        _cache[key] = ssw.Fsg.read(model, lex, C.fsg_path(grammar))
    return _cache[key]


def _search(model, lex, scr_list, plan, fsg_of_utt=None):
    off = np.concatenate([[0], np.cumsum([len(s) for s in scr_list])]).astype(np.int32)
    rows = np.concatenate(scr_list) if scr_list else np.zeros((0, model.n_sen), np.int16)
    d = torch.from_numpy(np.ascontiguousarray(rows, np.int16)).cuda()
    return ssw.grammar_search_batch(model, lex, d, off, plan, fsg_of_utt)


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


def _models(gpu_en, gpu_fr):
    return {"en-us": gpu_en, "fr-fr": gpu_fr}


@pytest.mark.parametrize("name", [c[0] for c in C.CASES])
def test_fixture_case(gpu_en, gpu_fr, name):
    """every case the reference recorded, one utterance per call"""
    _, _, grammar, mname, recording, samples = next(c for c in C.CASES if c[0] == name)
    model = _models(gpu_en, gpu_fr)[mname]
    lex = _lex(model, mname)
    scr = _scores(model, mname, recording, samples)
    assert len(scr) + 1 == RESULTS[name]["frames"]      # decoder_n_frames counts one more
    plan = lex.grammar_plan(_fsg(model, lex, mname, grammar))
    r = _search(model, lex, [scr], plan)
    got = _record(r, 0)
    print(name, got)
    assert got == _expected(name)


def test_all_en_us_cases_in_one_call(gpu_en):
    """per-utterance grammars, ragged lengths and the two-frame utterance in one batch: the same
    as one per call"""
    lex = _lex(gpu_en, "en-us")
    cases = [c for c in C.CASES if c[3] == "en-us"]
    grammars = sorted({c[2] for c in cases})
    plan = lex.grammar_plan([_fsg(gpu_en, lex, "en-us", g) for g in grammars])
    scr = [_scores(gpu_en, "en-us", c[4], c[5]) for c in cases]
    r = _search(gpu_en, lex, scr, plan, [grammars.index(c[2]) for c in cases])
    for u, c in enumerate(cases):
        assert _record(r, u) == _expected(c[0]), c[0]


@pytest.mark.parametrize("n_words,lo,hi", [(22, 257, 512), (40, 513, 1024), (50, 1025, 2048),
                                          (110, 2049, 4096)])
def test_every_instance_of_the_kernel(gpu_en, n_words, lo, hi):
    """the plan's largest grammar picks the kernel instance (256, 512, 1024 threads with one HMM
    each, then four and eight HMMs per thread): beside a loop grammar of the right size the
    mandatory grammars give what they give alone, and the loop grammar itself gives what the
    reference gave where it was recorded (50 and 110 words)"""
    lex = _lex(gpu_en, "en-us")
    scr = _scores(gpu_en, "en-us", "goforward.raw", 0)
    src = "loop110" if n_words > 50 else "loop50"
    _, _, _, _, trans = C.parse_fsg(C.fsg_path(src))
    pad = ssw.Fsg.create(gpu_en, lex, "pad", 0, 0,
                         [(0, 0, t[2], t[3]) for t in trans[:n_words]])
    names = ["goforward", "nulls", "loop"]
    plan = lex.grammar_plan([pad] + [_fsg(gpu_en, lex, "en-us", g) for g in names])
    assert lo <= plan.hmms(0) <= hi and max(plan.hmms(i) for i in (1, 2, 3)) < lo
    r = _search(gpu_en, lex, [scr] * 4, plan, [1, 2, 3, 0])
    for u, g in enumerate(names):
        assert _record(r, u) == _expected(g), g
    if n_words >= 50:
        assert len(trans) == n_words and _record(r, 3) == _expected(src)
    else:
        assert r.status(3) == 0 and r.hyp(3) == "go forward ten meters"


@pytest.mark.parametrize("grammar", ["goforward", "nulls"])
def test_one_grammar_shared_by_eight_utterances(gpu_en, grammar):
    lex = _lex(gpu_en, "en-us")
    scr = _scores(gpu_en, "en-us", "goforward.raw", 0)
    plan = lex.grammar_plan(_fsg(gpu_en, lex, "en-us", grammar))
    r = _search(gpu_en, lex, [scr] * 8, plan, None)
    for u in range(8):
        assert _record(r, u) == _expected(grammar), u
    r2 = _search(gpu_en, lex, [scr] * 8, plan, None)     # the plan's tables are on the device now
    assert [_record(r2, u) for u in range(8)] == [_record(r, u) for u in range(8)]


@pytest.mark.parametrize("text", ["go forward ten meters", "hello world", "ten",
                                  "go go forward ten meters meters"])
def test_chain_grammar_matches_first_pass(gpu_en, text):
    """a chain FSG of a text is the linear grammar of decoder_set_align_text: the grammar
    instance gives the words, frames and path scores ssw_first_pass_batch gives on the same rows"""
    lex = _lex(gpu_en, "en-us")
    words = text.split()
    scr = _scores(gpu_en, "en-us", "goforward.raw", 0)
    d = torch.from_numpy(scr).cuda()
    want = lex.first_pass(d, [0, len(scr)], [words])[0]
    fsg = ssw.Fsg.create(gpu_en, lex, "chain", 0, len(words),
                         [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    r = _search(gpu_en, lex, [scr], lex.grammar_plan(fsg))
    if want is None:
        assert r.status(0) == 1 and r.segments(0) == [] and r.hyp(0) is None
        assert r.message(0) == "Final result does not match the grammar in frame %d" % len(scr)
        return
    assert r.status(0) == 0
    got, total = [], 0
    for w, sf, ef, ascr, lscr in r.segments(0):
        total += ascr + lscr
        got.append((w, sf, ef - sf + 1, total))
    print(text, got)
    assert got == want
    assert r.score(0) == want[-1][3]


@pytest.mark.parametrize("mname,text", [("en-us", "go forward data ten meters"),
                                        ("fr-fr", "avance abus de ait dix mètres")])
def test_one_text_through_all_five_kernels(oracle_mod, gpu_en, gpu_fr, orc_en, orc_fr, monkeypatch,
                                           mname, text):
    """The five search kernels share every decision (ssw_search_common.inc) and differ in where the
    state lives: one text on ~150 frames of synthetic scores, searched as a linear text through
    first_pass_kernel, first_pass_win_kernel and first_pass_big_kernel and as its chain grammar
    through grammar_search_kernel and grammar_search_big_kernel (a plan that also holds a grammar
    beyond one workgroup is searched from the HBM workspace), gives the same words, frames and path
    scores five times.
    The en-us text has a word with an alternate ("data"); en-us lists no alternates pronounced
    alike, so the fr-fr text brings the twin records ("abus", "ait").  No reference here: each
    kernel is pinned to it by its own suite."""
    from oracle import fsg_oracle as F
    from tests.test_gpu_first_pass import synth_scores
    model, orc = (gpu_en, orc_en) if mname == "en-us" else (gpu_fr, orc_fr)
    lex = _lex(model, mname)
    d_ = os.path.join(MODEL_ROOT, mname)
    olex = F.Lexicon(orc, os.path.join(d_, "dict.txt"), os.path.join(d_, "noisedict.txt"))
    words = text.split()
    scr = synth_scores(F, orc, olex, words, 11, orc.n_sen)
    assert 100 <= len(scr) <= 250
    d = torch.from_numpy(scr).cuda()
    got = {}
    for kernel, env in (("first_pass_kernel", {}),
                        ("first_pass_win_kernel", {"SSW_FP_KERNEL": "big", "SSW_FP_WIN_TPB": "256"}),
                        ("first_pass_big_kernel", {"SSW_FP_KERNEL": "big", "SSW_FP_WIN": "0"})):
        with monkeypatch.context() as mp:
            for k, v in env.items():
                mp.setenv(k, v)
            got[kernel] = lex.first_pass(d, [0, len(scr)], [words])[0]
    chain = ssw.Fsg.create(model, lex, "chain", 0, len(words),
                           [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    plans = {"grammar_search_kernel": (lex.grammar_plan(chain), None)}
    if mname == "en-us":
        big = _fsg(model, lex, mname, "loop200")
    else:                       # (loop200 is an en-us grammar: a loop over 1000 fr-fr words)
        pad = [lex.word(i) for i in range(200, 1400)]
        pad = [w for w in pad if w and "(" not in w and not w.startswith("<")][:1000]
        big = ssw.Fsg.create(model, lex, "pad", 0, 0, [(0, 0, 1.0 / len(pad), w) for w in pad])
    plans["grammar_search_big_kernel"] = (lex.grammar_plan([chain, big], max_hmms=30000), [0])
    assert plans["grammar_search_big_kernel"][0].hmms(1) > 4096
    for kernel, (plan, which) in plans.items():
        r = _search(model, lex, [scr], plan, which)
        assert r.status(0) == 0, kernel
        segs, total = [], 0
        for w, sf, ef, ascr, lscr in r.segments(0):
            total += ascr + lscr
            segs.append((w, sf, ef - sf + 1, total))
        assert r.score(0) == total, kernel
        got[kernel] = segs
    for kernel, segs in got.items():
        print(kernel, segs)
    want = got["first_pass_kernel"]
    assert want is not None and len(want) >= len(words)
    for kernel, segs in got.items():
        assert segs == want, kernel


@pytest.mark.parametrize("mname,recording,case", [("en-us", "goforward.raw", "goforward"),
                                                  ("fr-fr", "goforward_fr.raw", "fr")])
def test_recognize_audio_batch(gpu_en, gpu_fr, mname, recording, case):
    """PCM in, the reference's JSON line out: front end, features, scores and search in one call"""
    model = _models(gpu_en, gpu_fr)[mname]
    lex = _lex(model, mname)
    pcm = C.pcm(recording, 0)
    plan = lex.grammar_plan(_fsg(model, lex, mname, RESULTS[case]["grammar"]))
    r = ssw.recognize_audio_batch(model, lex, pcm, [0, len(pcm)], plan)
    assert r.json(0) == RESULTS[case]["json"]
    assert r.hyp(0) == RESULTS[case]["hyp"] and r.score(0) == RESULTS[case]["score"]


def test_two_recordings_of_one_batch_from_audio(gpu_en):
    """ragged audio batch, two grammars"""
    lex = _lex(gpu_en, "en-us")
    full, cut = C.pcm("goforward.raw", 0), C.pcm("goforward.raw", 19200)
    plan = lex.grammar_plan([_fsg(gpu_en, lex, "en-us", "loop"),
                             _fsg(gpu_en, lex, "en-us", "goforward")])
    r = ssw.recognize_audio_batch(gpu_en, lex, np.concatenate([full, cut]),
                                  [0, len(full), len(full) + len(cut)], plan, [1, 0])
    assert r.json(0) == RESULTS["goforward"]["json"]
    assert r.json(1) == RESULTS["loop_1200ms"]["json"]


def test_grammar_over_the_hmm_limit_is_refused(gpu_en):
    """more phone-tree HMMs than one workgroup holds: refused when the plan is made, before any
    launch, naming the count and the limit"""
    lex = _lex(gpu_en, "en-us")
    words = [lex.word(i) for i in range(200, 3200)]
    words = [w for w in words if w and "(" not in w and not w.startswith("<")]
    fsg = ssw.Fsg.create(gpu_en, lex, "big", 0, 0, [(0, 0, 1.0 / len(words), w) for w in words])
    with pytest.raises(ssw.SswError, match=r"has \d+ phone-tree HMMs: the grammar search holds at "
                                           r"most 4096"):
        lex.grammar_plan(fsg)


def test_history_budget_is_enforced(gpu_en, monkeypatch):
    lex = _lex(gpu_en, "en-us")
    scr = _scores(gpu_en, "en-us", "goforward.raw", 0)
    plan = lex.grammar_plan(_fsg(gpu_en, lex, "en-us", "goforward"))
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "1")
    with pytest.raises(ssw.SswError, match="exceeds the budget"):
        _search(gpu_en, lex, [scr] * 64, plan)
