"""Phone and state times for recognised speech on the GPU: ssw_recognition_set_align,
ssw_recognize_align_batch (compallsen = yes) and ssw_recognize_align_batch_active (compallsen = no,
the reference's default), against what the reference library printed for decoder_result_json at
align_level 1 and 2 and listed for decoder_alignment after the same grammars
(tests/golden/fsg_align_results.json, written by tests/golden/make_fsg_align.py from
tests/harness/fsg_align_driver.c), and against the project's own text alignment and hand-made
chains.

Nothing is tolerated: status, message, the JSON lines byte for byte and every (start, duration,
score) are compared for equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from soundswallower_amd.api import _ptr
from tests import cont_common as CC
from tests import fsg_align_common as A
from tests import fsg_common as F
from tests import sc_common as S
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

RESULTS = A.results()
NO_EXIT = "No hypothesis: no word exit in any frame"
_cache = {}


@pytest.fixture(scope="module")
def models(gpu_en, gpu_fr, tmp_path_factory):
    """name -> (Model, Lexicon): the two shipped models, the semi-continuous one and C3"""
    tmp = str(tmp_path_factory.mktemp("recognize_align"))
    sc = S.model_a_dir(os.path.join(tmp, "cb41"))
    c3 = CC.BUILDERS["C3"](os.path.join(tmp, "C3"))
    got = {"en-us": (gpu_en, os.path.join(MODEL_ROOT, "en-us")),
           "fr-fr": (gpu_fr, os.path.join(MODEL_ROOT, "fr-fr")),
           "cb41": (ssw.Model(sc), sc), "C3": (ssw.Model(**CC.model_paths(c3)), c3)}
    assert got["cb41"][0].scorer() == ssw.SCORER_S2_SEMI and got["C3"][0].continuous
    return {k: (m, ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt")))
            for k, (m, d) in got.items()}


def _feats(model, mname, recording, samples):
    """feature rows of the first `samples` samples of a recording, once per session"""
    key = ("feat", mname, recording, samples)
    if key not in _cache:
        cep, _ = model.fe_batch(F.pcm(recording, samples))
        _cache[key] = np.ascontiguousarray(model.feat_batch(cep), np.float32)
    return _cache[key]


def _plan(models, case, config):
    """the plan of a fixture case; a large grammar gets one of its own (flagged for the default
    configuration)"""
    _, kind, grammar, mname, _, _ = case
    key = ("plan", kind, grammar, mname, config if kind == "large" else "")
    if key not in _cache:
        model, lex = models[mname]
        fsg = (ssw.Fsg.from_jsgf(model, lex, path=A.grammar_path(case)) if kind == "jsgf"
               else ssw.Fsg.read(model, lex, A.grammar_path(case)))
        _cache[key] = (lex.grammar_plan(fsg, max_hmms=A.MAX_HMMS, active=config == "no")
                       if kind == "large" else lex.grammar_plan(fsg))
    return _cache[key]


def _run(model, lex, feat_list, plan, config, fsg_of_utt=None, two_pass_history=False):
    """(RecognitionSet, AlignmentSet, rounds or None) of the new call for a configuration"""
    off = np.concatenate([[0], np.cumsum([len(f) for f in feat_list])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(feat_list)).cuda()
    if config == "no":
        return ssw.recognize_align_batch_active(model, lex, d, off, plan, fsg_of_utt,
                                                two_pass_history=two_pass_history)
    return ssw.recognize_align_batch(model, lex, d, off, plan, fsg_of_utt,
                                     two_pass_history=two_pass_history) + (None,)


def _entries(al, u):
    """utterance u of an AlignmentSet: status, message, and the alignment in the fixture's terms"""
    got = {"status": al.status(u), "message": al.message(u)}
    x = al.utterance(u)
    if x is None:
        with pytest.raises(ssw.SswError, match="ssw_alignment_set_json"):
            al.json(u, align_level=1)
        return got
    got.update(json1=al.json(u, align_level=1), json2=al.json(u, align_level=2),
               words=[[w] + [int(v) for v in e] for w, e in zip(x["words"], x["word_al"])],
               phones=[[int(v) for v in e] for e in x["phone_al"]],
               states=[[str(int(s))] + [int(v) for v in e]
                       for s, e in zip(x["senid"].reshape(-1), x["state_al"])])
    return got


def _expected(key):
    fx = RESULTS[key]
    if fx["json1"] is None:
        return {"status": 1, "message": fx["errors"][-1] if fx["errors"] else NO_EXIT}
    return {"status": 0, "message": "", "json1": fx["json1"], "json2": fx["json2"],
            "words": fx["words"], "phones": [p[1:] for p in fx["phones"]], "states": fx["states"]}


def _rec(r, u):
    return {"status": r.status(u), "message": r.message(u), "hyp": r.hyp(u), "score": r.score(u),
            "segments": [list(s) for s in r.segments(u)], "json": r.json(u)}


# ------------------------------------------------------------------------------------------
# 1 and 6: the reference's records
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", A.keys())
def test_fixture_case(models, key):
    """every recorded case under its configuration, with two_pass_history 0 and 1 (the reference
    keeps its history across the two passes; on these recordings the two give the same numbers)"""
    name, config = key.split("/")
    case = A.case(name)
    model, lex = models[case[3]]
    feats = _feats(model, case[3], case[4], case[5])
    fx = RESULTS[key]
    assert len(feats) + 1 == fx["frames"]      # decoder_n_frames counts one more
    plan = _plan(models, case, config)
    for tph in (0, 1):
        r, al, rounds = _run(model, lex, [feats], plan, config, two_pass_history=tph)
        got = _entries(al, 0)
        print(key, "two_pass_history", tph, "rounds", None if rounds is None else rounds.tolist(),
              got["status"], got["message"])
        assert got == _expected(key), tph
        assert (r.hyp(0), r.score(0), r.json(0)) == (fx["hyp"], fx["score"], fx["json0"])
        r.free()
        al.free()


def test_continuous_model_is_refused_by_name_in_the_default_configuration(models):
    model, lex = models["C3"]
    case = A.case("cont_goforward")
    feats = _feats(model, "C3", case[4], case[5])
    with pytest.raises(ssw.SswError, match="continuous") as e:
        _run(model, lex, [feats], _plan(models, case, "yes"), "no")
    assert "ssw_recognize_align_batch_active" in str(e.value)
    r, al, _ = _run(model, lex, [feats], _plan(models, case, "yes"), "yes")
    assert _entries(al, 0) == _expected("cont_goforward/yes")


def test_s2_semi_default_configuration_takes_the_whole_rows_route(models):
    model, lex = models["cb41"]
    case = A.case("sc_goforward")
    feats = _feats(model, "cb41", case[4], case[5])
    plan = _plan(models, case, "yes")
    for tph in (0, 1):
        r0, a0, _ = _run(model, lex, [feats], plan, "yes", two_pass_history=tph)
        r1, a1, rounds = _run(model, lex, [feats], plan, "no", two_pass_history=tph)
        assert _entries(a0, 0) == _entries(a1, 0) and _entries(a0, 0)["status"] == 0
        assert _rec(r0, 0) == _rec(r1, 0) and rounds.tolist() == [1]


def test_audio_entry(models):
    """recognize_align_audio_batch: PCM in, the recorded lines out, in both configurations"""
    model, lex = models["en-us"]
    case = A.case("goforward")
    pcm = F.pcm(case[4], case[5])
    for config in A.CONFIGS:
        r, al = ssw.recognize_align_audio_batch(model, lex, pcm, [0, len(pcm)],
                                                _plan(models, case, config), active=config == "no")
        assert _entries(al, 0) == _expected("goforward/" + config)
        assert r.json(0) == RESULTS["goforward/" + config]["json0"]


# ------------------------------------------------------------------------------------------
# 2: rec_out is the existing calls' set
# ------------------------------------------------------------------------------------------
def test_rec_out_equals_the_recognition_calls(models):
    model, lex = models["en-us"]
    names = ("goforward", "loop", "nulls", "nomatch", "goforward_1200ms", "loop_410")
    cases = [A.case(n) for n in names]
    grammars = sorted({c[2] for c in cases})
    plan = lex.grammar_plan([ssw.Fsg.read(model, lex, F.fsg_path(g)) for g in grammars])
    feats = [_feats(model, "en-us", c[4], c[5]) for c in cases]
    which = [grammars.index(c[2]) for c in cases]
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(feats)).cuda()
    want = ssw.recognize_batch(model, lex, d, off, plan, which)
    want_no, want_rounds = ssw.recognize_batch_active(model, lex, d, off, plan, which)
    for tph in (0, 1):
        r, al, _ = _run(model, lex, feats, plan, "yes", which, tph)
        r_no, al_no, rounds = _run(model, lex, feats, plan, "no", which, tph)
        for u in range(len(cases)):
            assert _rec(r, u) == _rec(want, u), (tph, names[u])
            assert _rec(r_no, u) == _rec(want_no, u), (tph, names[u])
        assert rounds.tolist() == want_rounds.tolist()
        assert [al.status(u) for u in range(len(cases))] == [0, 0, 0, 1, 1, 1]
        assert [al_no.status(u) for u in range(len(cases))] == [0, 0, 0, 1, 1, 1]


# ------------------------------------------------------------------------------------------
# 3: batches
# ------------------------------------------------------------------------------------------
BATCHES = {
    1: ("goforward",),
    2: ("loop_1200ms", "nulls"),
    # whole and truncated recordings, a two-frame one, nomatch in the middle, a duplicate
    7: ("goforward", "loop", "nulls", "nomatch", "loop_1200ms", "goforward_410", "goforward"),
}


@pytest.mark.parametrize("config", A.CONFIGS)
@pytest.mark.parametrize("n", sorted(BATCHES))
def test_batches_equal_the_utterances_alone(models, n, config):
    model, lex = models["en-us"]
    cases = [A.case(name) for name in BATCHES[n]]
    grammars = ["goforward", "loop", "nulls", "nomatch"]
    key = ("plan4",)
    if key not in _cache:
        _cache[key] = lex.grammar_plan([ssw.Fsg.read(model, lex, F.fsg_path(g)) for g in grammars])
    plan = _cache[key]
    feats = [_feats(model, "en-us", c[4], c[5]) for c in cases]
    which = [grammars.index(c[2]) for c in cases]
    alone = []
    for c, f, w in zip(cases, feats, which):
        k = ("alone", c[0], config)
        if k not in _cache:
            r, al, _ = _run(model, lex, [f], plan, config, [w])
            _cache[k] = _entries(al, 0)
            assert _cache[k] == _expected(c[0] + "/" + config)
        alone.append(_cache[k])
    for tph in (0, 1):
        r, al, _ = _run(model, lex, feats, plan, config, which, tph)
        for u, c in enumerate(cases):
            assert _entries(al, u) == alone[u], (tph, c[0])
    if n == 7:
        assert [al.status(u) for u in range(7)] == [0, 0, 0, 1, 0, 1, 0]
        assert al.message(3) == r.message(3) and "does not match the grammar" in al.message(3)
        assert al.message(5) == r.message(5) == NO_EXIT


# ------------------------------------------------------------------------------------------
# 4: the chain done by hand, whole rows
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grammars", [("goforward",), ("nulls", "nomatch", "loop")])
def test_recognition_set_align_equals_the_chain_by_hand(models, grammars):
    """RecognitionSet.align after grammar_search_batch = ssw_alignment_populate over the set's
    dictionary-word segments, ssw_align_batch within those windows, ssw_alignment_propagate"""
    model, lex = models["en-us"]
    feats = _feats(model, "en-us", "goforward.raw", 0)
    T, n = len(feats), len(grammars)
    scr = model.score_batch(np.concatenate([feats] * n), (np.arange(n + 1) * T).astype(np.int32))
    d = torch.from_numpy(np.ascontiguousarray(scr)).cuda()
    off = (np.arange(n + 1) * T).astype(np.int32)
    plan = lex.grammar_plan([ssw.Fsg.read(model, lex, F.fsg_path(g)) for g in grammars])
    r = ssw.grammar_search_batch(model, lex, d, off, plan, list(range(n)))
    al = r.align(model, d, off)
    sseq = model.table("sseq").reshape(-1, 3)
    for u, g in enumerate(grammars):
        if r.status(u) != 0:
            assert g == "nomatch" and al.status(u) == 1 and al.message(u) == r.message(u)
            continue
        segs = [s for s in r.segments(u) if s[0] != "(NULL)"]
        if g == "nulls":     # "(NULL)" entries on the path: skipped, as decoder_alignment does
            assert len(segs) < len(r.segments(u))
        p = lex.populate([s[0] for s in segs], [s[1] for s in segs], [s[2] - s[1] + 1 for s in segs])
        n_ph = len(p["ssid"])
        init = np.zeros((n_ph * 3, 3), np.int32)
        init[:, 0], init[:, 1] = np.repeat(p["start"], 3), np.repeat(p["duration"], 3)
        states, status = model.align_batch(d[u * T:(u + 1) * T], [0, T], [0, n_ph], sseq[p["ssid"]],
                                           p["tmatid"], sf=p["start"], ef=p["start"] + p["duration"],
                                           state_init=init)
        assert status[0] == 0
        phones = model.propagate(states, np.repeat(np.arange(n_ph), 3), n_ph)
        words = model.propagate(phones, p["parent"], len(segs))
        x = al.utterance(u)
        assert x["words"] == [s[0] for s in segs]
        assert np.array_equal(x["cipid"], p["cipid"]) and np.array_equal(x["parent"], p["parent"])
        assert np.array_equal(x["senid"], sseq[p["ssid"]])
        assert np.array_equal(x["state_al"], states)
        assert np.array_equal(x["phone_al"], phones) and np.array_equal(x["word_al"], words)
        assert [(int(s), int(n_)) for s, n_, _ in x["word_al"]] == [(s[1], s[2] - s[1] + 1) for s in segs]


# ------------------------------------------------------------------------------------------
# 5: the linear grammar against the text alignment
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("config", A.CONFIGS)
@pytest.mark.parametrize("tph", (0, 1))
def test_linear_grammar_equals_text_alignment(models, config, tph):
    model, lex = models["en-us"]
    words = "go forward ten meters".split()
    fsg = ssw.Fsg.create(model, lex, "chain", 0, len(words),
                         [(i, i + 1, 1.0, w) for i, w in enumerate(words)])
    plan = lex.grammar_plan(fsg)
    feats = [_feats(model, "en-us", "goforward.raw", 0), _feats(model, "en-us", "goforward.raw", 19200)]
    off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(feats)).cuda()
    cfg = lex.first_pass_config(two_pass_history=tph)
    text = ssw.align_text_batch_active if config == "no" else ssw.align_text_batch
    want = text(model, lex, d, off, [words] * 2, cfg=cfg)
    r, al, _ = _run(model, lex, feats, plan, config, two_pass_history=tph)
    assert want.status(0) == 0 and al.status(0) == 0
    for u in range(2):
        assert al.status(u) == want.status(u)
        if want.status(u) != 0:
            continue
        w = want.utterance(u)
        # the precondition: the two first passes found the same words in the same frames
        segs = [(s[0], s[1], s[2] - s[1] + 1) for s in r.segments(u) if s[0] != "(NULL)"]
        assert segs == [(n_, int(e[0]), int(e[1])) for n_, e in zip(w["words"], w["word_al"])], \
            "the first passes differ: nothing is said about the second"
        g = al.utterance(u)
        for k in ("wid", "word_al", "cipid", "parent", "phone_al", "senid", "state_al"):
            assert np.array_equal(g[k], w[k]), k
        for level in (1, 2):
            assert al.json(u, align_level=level) == want.json(u, align_level=level)


# ------------------------------------------------------------------------------------------
# 7: refusals
# ------------------------------------------------------------------------------------------
def test_refusals_leave_the_model_usable(models):
    model, lex = models["en-us"]
    fr, lex_fr = models["fr-fr"]
    L = _lib.lib()
    case = A.case("goforward")
    plan = _plan(models, case, "yes")
    feats = _feats(model, "en-us", case[4], case[5])
    T = len(feats)
    d = torch.from_numpy(feats).cuda()
    off = np.array([0, T], np.int32)
    scorer = model.pick_scorer(None)

    def ok():
        for config in A.CONFIGS:
            _, al, _ = _run(model, lex, [feats], plan, config)
            assert _entries(al, 0) == _expected("goforward/" + config)

    def raw(fn, plan_p, n_frames, *tail):
        rec = C.c_void_p()
        h = fn(model._m, lex._d, plan_p, None, scorer, _ptr(d), n_frames, _ptr(off), 1, 0,
               C.byref(rec), *tail)
        assert not h and not rec.value
        return _lib.last_error()

    # NULL plan; utt_off that does not span n_frames
    assert "bad arguments to ssw_recognize_align_batch" in raw(L.ssw_recognize_align_batch, None, T, None)
    assert "bad arguments to ssw_recognize_align_batch_active" in raw(
        L.ssw_recognize_align_batch_active, None, T, None, None)
    ok()
    assert "bad arguments to ssw_recognize_align_batch" in raw(L.ssw_recognize_align_batch, plan._p,
                                                               T - 1, None)
    assert "bad arguments to ssw_recognize_align_batch_active" in raw(
        L.ssw_recognize_align_batch_active, plan._p, T + 1, None, None)
    ok()
    # a recognition set from another model; frame counts that are not the set's
    scr = torch.from_numpy(np.ascontiguousarray(model.score_batch(feats))).cuda()
    fcase = A.case("fr")
    ffeats = _feats(fr, "fr-fr", fcase[4], fcase[5])
    r_fr, _, _ = _run(fr, lex_fr, [ffeats], _plan(models, fcase, "yes"), "yes")
    with pytest.raises(ssw.SswError, match="another model"):
        r_fr.align(model, scr, [0, len(ffeats)])
    r = ssw.grammar_search_batch(model, lex, scr, off, plan)
    with pytest.raises(ssw.SswError, match="frames in utt_off"):
        r.align(model, scr, [0, T - 1])
    with pytest.raises(ssw.SswError, match="utt_off"):
        r.align(model, scr, [0, 100, T])
    assert _entries(r.align(model, scr, off), 0) == _expected("goforward/yes")
    ok()
    # the default configuration with a large plan that was not made for it
    big = A.case("loop200")
    with pytest.raises(ssw.SswError, match="ssw_grammar_prepare_large_active") as e:
        _run(model, lex, [feats], _plan(models, big, "yes"), "no")
    assert "ssw_recognize_align_batch_active" in str(e.value) and "loop200" in str(e.value)
    ok()
