"""Recognition against word FSGs in the reference's DEFAULT configuration (compallsen = no) on the
GPU: ssw_recognize_batch_active, against what the reference library itself recognised with no
setting but its log level (tests/golden/fsg_default_results.json, written by
tests/golden/make_fsg_default.py from tests/harness/fsg_default_driver.c).

In that configuration acmod scores, frame by frame, only the senones of the HMMs the search holds
active, and the scorer normalises over them: frame t is scored after frame t - 1 was searched.
The batch call assumes the sets, scores the batch with them, searches again and accepts an
utterance whose search took exactly the assumed sets (ssw_k7_fpactive.inc, ssw_k9_grammar.inc).

Nothing is tolerated: status, message, words, frames, integer scores and the JSON line are compared
for equality."""
import json
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(C.GOLD, "fsg_default_results.json"), encoding="utf-8") as _f:
    RESULTS = json.load(_f)
RESULTS_YES = C.results()
_cache = {}


def _lex(model, name):
    key = ("lex", name)
    if key not in _cache:
        d = os.path.join(MODEL_ROOT, name)
        _cache[key] = ssw.Lexicon(model, os.path.join(d, "dict.txt"),
                                  os.path.join(d, "noisedict.txt"))
    return _cache[key]


def _feats(model, name, recording, samples):
    """feature rows of the first `samples` samples of a recording: front end and dynamic features
    on the GPU, once per session"""
    key = ("feat", name, recording, samples)
    if key not in _cache:
        cep, _ = model.fe_batch(C.pcm(recording, samples))
        _cache[key] = np.ascontiguousarray(model.feat_batch(cep), np.float32)
    return _cache[key]


def _fsg(model, lex, name, grammar):
    key = ("fsg", name, grammar)
    if key not in _cache:
        _cache[key] = ssw.Fsg.read(model, lex, C.fsg_path(grammar))
    return _cache[key]


def _recognize(model, lex, feat_list, plan, fsg_of_utt=None, **kw):
    off = np.concatenate([[0], np.cumsum([len(f) for f in feat_list])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(feat_list)).cuda()
    return ssw.recognize_batch_active(model, lex, d, off, plan, fsg_of_utt, **kw)


def _record(r, u):
    """utterance u of a RecognitionSet in the fixture's terms"""
    return {"status": r.status(u), "message": r.message(u), "hyp": r.hyp(u), "score": r.score(u),
            "segments": [list(s) for s in r.segments(u)], "json": r.json(u)}


def _expected(name, results=RESULTS):
    fx = results[name]
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
    """every case the reference recorded under its defaults, one utterance per call.  Both models
    are scored by the PTM scorer, the one the reference's acmod_init picks for them (it tries
    ptm_mgau_init first)."""
    _, _, grammar, mname, recording, samples = next(c for c in C.CASES if c[0] == name)
    model = _models(gpu_en, gpu_fr)[mname]
    lex = _lex(model, mname)
    feats = _feats(model, mname, recording, samples)
    assert len(feats) + 1 == RESULTS[name]["frames"]      # decoder_n_frames counts one more
    plan = lex.grammar_plan(_fsg(model, lex, mname, grammar))
    r, rounds = _recognize(model, lex, [feats], plan)
    got = _record(r, 0)
    print(name, "rounds", rounds.tolist(), got)
    assert got == _expected(name)
    assert rounds[0] >= 1


def test_all_en_us_cases_in_one_call(gpu_en):
    """per-utterance grammars, ragged lengths and the two-frame utterances in one batch: the same
    as one per call, with the rounds over the unproven utterances taken every way the loop can"""
    lex = _lex(gpu_en, "en-us")
    cases = [c for c in C.CASES if c[3] == "en-us"]
    grammars = sorted({c[2] for c in cases})
    plan = lex.grammar_plan([_fsg(gpu_en, lex, "en-us", g) for g in grammars])
    feats = [_feats(gpu_en, "en-us", c[4], c[5]) for c in cases]
    which = [grammars.index(c[2]) for c in cases]
    r, rounds = _recognize(gpu_en, lex, feats, plan, which)
    print("rounds per utterance:", rounds.tolist())
    for u, c in enumerate(cases):
        assert _record(r, u) == _expected(c[0]), c[0]
        assert len(feats[u]) > 0 and rounds[u] >= 1, c[0]
    for sub in ("0", "1"):
        os.environ["SSW_FPA_SUB"] = sub
        try:
            r2, rounds2 = _recognize(gpu_en, lex, feats, plan, which)
        finally:
            del os.environ["SSW_FPA_SUB"]
        print("SSW_FPA_SUB=%s rounds per utterance:" % sub, rounds2.tolist())
        for u, c in enumerate(cases):
            assert _record(r2, u) == _expected(c[0]), (sub, c[0])
            assert rounds2[u] >= 1, (sub, c[0])


@pytest.mark.parametrize("n_words,lo,hi", [(22, 257, 512), (40, 513, 1024), (50, 1025, 2048),
                                          (110, 2049, 4096)])
def test_every_instance_of_the_kernel(gpu_en, n_words, lo, hi):
    """the plan's largest grammar picks the kernel instance (256, 512, 1024 threads with one HMM
    each, then four and eight HMMs per thread), here the ones that export their sets: beside a
    loop grammar of the right size the mandatory grammars give what they give alone, and the loop
    grammar itself gives what the reference gave where it was recorded (50 and 110 words).  The
    256-thread instance is the one test_fixture_case runs."""
    lex = _lex(gpu_en, "en-us")
    feats = _feats(gpu_en, "en-us", "goforward.raw", 0)
    src = "loop110" if n_words > 50 else "loop50"
    _, _, _, _, trans = C.parse_fsg(C.fsg_path(src))
    pad = ssw.Fsg.create(gpu_en, lex, "pad", 0, 0,
                         [(0, 0, t[2], t[3]) for t in trans[:n_words]])
    names = ["goforward", "nulls", "loop"]
    plan = lex.grammar_plan([pad] + [_fsg(gpu_en, lex, "en-us", g) for g in names])
    assert lo <= plan.hmms(0) <= hi and max(plan.hmms(i) for i in (1, 2, 3)) < lo
    r, rounds = _recognize(gpu_en, lex, [feats] * 4, plan, [1, 2, 3, 0])
    print("rounds per utterance:", rounds.tolist())
    for u, g in enumerate(names):
        assert _record(r, u) == _expected(g), g
    if n_words >= 50:
        assert len(trans) == n_words and _record(r, 3) == _expected(src)
    else:
        # no reference record of these sizes: the pad grammar alone in the plan (the same kernel
        # instance, another batch) gives the same
        alone, _ = _recognize(gpu_en, lex, [feats], lex.grammar_plan(pad))
        assert r.status(3) == 0 and _record(r, 3) == _record(alone, 0)


def _flags2list(O, bits, n_sen):
    return O.flags2list(np.ascontiguousarray(bits, np.uint32), n_sen)


def test_rows_are_the_references_scores_and_close_the_loop(gpu_en, orc_en, oracle_mod):
    """goforward with the rows and the listed senones returned: walking the frames in order, every
    listed senone's score is what the CPU oracle's restatement of ptm_mgau_frame_eval gives for
    that frame's list (compallsen = no); and the plain grammar search over those rows -- which
    reads only listed entries -- gives the same record."""
    O = oracle_mod
    lex = _lex(gpu_en, "en-us")
    feats = _feats(gpu_en, "en-us", "goforward.raw", 0)
    n = len(feats)
    plan = lex.grammar_plan(_fsg(gpu_en, lex, "en-us", "goforward"))
    d_rows = torch.zeros((n, gpu_en.n_sen), dtype=torch.int16, device="cuda")
    r, rounds, listed = _recognize(gpu_en, lex, [feats], plan, d_senscr=d_rows, want_listed=True)
    torch.cuda.synchronize()
    assert _record(r, 0) == _expected("goforward")
    rows = d_rows.cpu().numpy()
    assert listed.shape == (n, (gpu_en.n_sen + 31) // 32)
    orc_en.ptm_reset()
    orc_en.ptm_set_frame_idx(0)
    for f in range(n):
        lst = _flags2list(O, listed[f], orc_en.n_sen)
        want = orc_en.ptm_frame_eval(feats[f], f, compallsen=False, senone_active=lst)
        orc_en.ptm_set_frame_idx(f + 1)
        sen = np.flatnonzero((listed[f][:, None] >> np.arange(32, dtype=np.uint32)) & 1)
        assert len(sen) > 0, f
        assert np.array_equal(rows[f][sen], np.asarray(want)[sen]), f
    # closure
    off = np.array([0, n], np.int32)
    again = ssw.grammar_search_batch(gpu_en, lex, d_rows, off, plan)
    assert _record(again, 0) == _record(r, 0)


@pytest.mark.parametrize("mname,recording,case", [("en-us", "goforward.raw", "goforward"),
                                                  ("fr-fr", "goforward_fr.raw", "fr")])
def test_recognize_audio_batch_active(gpu_en, gpu_fr, mname, recording, case):
    """PCM in, the reference's JSON line out: active=True gives the default configuration's,
    active=False still the compallsen = yes one"""
    model = _models(gpu_en, gpu_fr)[mname]
    lex = _lex(model, mname)
    pcm = C.pcm(recording, 0)
    plan = lex.grammar_plan(_fsg(model, lex, mname, RESULTS[case]["grammar"]))
    r = ssw.recognize_audio_batch(model, lex, pcm, [0, len(pcm)], plan, active=True)
    assert r.json(0) == RESULTS[case]["json"]
    assert r.hyp(0) == RESULTS[case]["hyp"] and r.score(0) == RESULTS[case]["score"]
    r = ssw.recognize_audio_batch(model, lex, pcm, [0, len(pcm)], plan, active=False)
    assert r.json(0) == RESULTS_YES[case]["json"]
    assert r.score(0) == RESULTS_YES[case]["score"] != RESULTS[case]["score"]


def test_stats_grow_by_what_the_call_reported(gpu_en):
    lex = _lex(gpu_en, "en-us")
    feats = _feats(gpu_en, "en-us", "goforward.raw", 0)
    cut = _feats(gpu_en, "en-us", "goforward.raw", 19200)
    plan = lex.grammar_plan([_fsg(gpu_en, lex, "en-us", "loop"),
                             _fsg(gpu_en, lex, "en-us", "goforward")])
    before = gpu_en.grammar_active_stats()
    fp_before = gpu_en.first_pass_active_stats()
    r, rounds = _recognize(gpu_en, lex, [feats, cut, feats], plan, [1, 0, 0])
    after = gpu_en.grammar_active_stats()
    assert after[0] - before[0] == 3
    assert after[1] - before[1] == int(rounds.sum())
    assert after[2] == int(rounds.max())
    assert after[3] - before[3] == int((rounds > 1).sum())
    assert gpu_en.first_pass_active_stats() == fp_before   # the first pass's counters are its own
    assert _record(r, 1) == _expected("loop_1200ms")


def test_frame_downsampling_is_refused():
    """ds != 1 with the PTM scorer: refused with the limit's message, before anything is uploaded
    or launched"""
    mdir = ssw.model_dir("en-us")
    g = ssw.Model(mdir, config={"ds": 2})
    lex = ssw.Lexicon(g, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    plan = lex.grammar_plan(ssw.Fsg.read(g, lex, C.fsg_path("goforward")))
    d = torch.zeros((4, 39), dtype=torch.float32, device="cuda")
    before = g.grammar_active_stats()
    with pytest.raises(ssw.SswError, match=r"ssw_recognize_batch_active: frame down-sampling "
                                           r"\(ds != 1\)"):
        ssw.recognize_batch_active(g, lex, d, [0, 4], plan)
    assert g.grammar_active_stats() == before
