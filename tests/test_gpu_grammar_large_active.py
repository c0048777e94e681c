"""Recognition against grammars of more than 4096 phone-tree HMMs in the reference's DEFAULT
configuration (compallsen = no) on the GPU: ssw_recognize_batch_active on a plan made by
ssw_grammar_prepare_large_active (grammar_search_big_kernel<1024, EXPORT>), against what the
reference library itself recognised with no setting but its log level
(tests/golden/fsg_large_default_results.json, written by make_fsg_large_default.py), and the
committed small default truths (fsg_default_results.json) searched by the same kernel.

Nothing is tolerated: status, message, words, frames, integer scores and the JSON line are compared
for equality."""
import json
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fsg_common as C
from tests import fsg_large_common as CL
from tests import fsg_large_default_common as CD
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

with open(os.path.join(C.GOLD, "fsg_default_results.json"), encoding="utf-8") as _f:
    RESULTS = dict(json.load(_f), **CD.results())       # compallsen = no, small and large
RESULTS_YES = dict(C.results(), **CL.results())
_cache = {}


def _lex(model):
    if "lex" not in _cache:
        d = os.path.join(MODEL_ROOT, "en-us")
        _cache["lex"] = ssw.Lexicon(model, os.path.join(d, "dict.txt"),
                                    os.path.join(d, "noisedict.txt"))
    return _cache["lex"]


def _feats(model, samples):
    """feature rows of the first `samples` samples of goforward.raw: front end and dynamic
    features on the GPU, once per session"""
    key = ("feat", samples)
    if key not in _cache:
        cep, _ = model.fe_batch(C.pcm("goforward.raw", samples))
        _cache[key] = np.ascontiguousarray(model.feat_batch(cep), np.float32)
    return _cache[key]


def _fsg(model, grammar):
    key = ("fsg", grammar)
    if key not in _cache:
        _cache[key] = ssw.Fsg.read(model, _lex(model), C.fsg_path(grammar))
    return _cache[key]


def _plan(model, grammars):
    """one flagged plan per list of grammars, kept: its tables stay on the device between tests"""
    key = ("plan", tuple(grammars))
    if key not in _cache:
        _cache[key] = _lex(model).grammar_plan([_fsg(model, g) for g in grammars],
                                               max_hmms=30000, active=True)
        assert _cache[key].active
    return _cache[key]


def _recognize(model, feat_list, plan, fsg_of_utt=None, **kw):
    off = np.concatenate([[0], np.cumsum([len(f) for f in feat_list])]).astype(np.int32)
    d = torch.from_numpy(np.concatenate(feat_list)).cuda()
    return ssw.recognize_batch_active(model, _lex(model), d, off, plan, fsg_of_utt, **kw)


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


@pytest.mark.parametrize("name", [c[0] for c in CL.CASES])
def test_large_default_fixture_case(gpu_en, name):
    """every case the reference recorded under its defaults, one utterance per call"""
    _, _, grammar, _, _, samples = next(c for c in CL.CASES if c[0] == name)
    feats = _feats(gpu_en, samples)
    assert len(feats) + 1 == RESULTS[name]["frames"]      # decoder_n_frames counts one more
    plan = _plan(gpu_en, [grammar])
    assert plan.hmms(0) == CL.HMMS[grammar]
    r, rounds = _recognize(gpu_en, [feats], plan)
    got = _record(r, 0)
    print(name, "rounds", rounds.tolist(), got)
    assert got == _expected(name)
    assert rounds[0] >= 1


def test_the_small_default_truths_on_the_large_kernel(gpu_en):
    """one grammar beyond the one-workgroup limits puts the whole plan on the HBM-workspace
    kernel: start-state nulls, no match, silence, twins and the two-frame truncations give their
    committed default-configuration records there, and loop200 beside them its own; with the
    rounds over the unproven utterances taken every way the loop can (the subset launches)"""
    grammars = ["loop200", "goforward", "nulls", "loop", "sil", "nomatch"]
    plan = _plan(gpu_en, grammars)
    cases = [("loop200", "loop200", 0)] + [(g, g, 0) for g in grammars[1:]]
    cases += [(c[0], c[2], c[5]) for c in C.CASES if c[0] in ("goforward_410", "loop_410")]
    assert len(cases) == 8
    feats = [_feats(gpu_en, s) for _, _, s in cases]
    which = [grammars.index(g) for _, g, _ in cases]
    r, rounds = _recognize(gpu_en, feats, plan, which)
    print("rounds per utterance:", rounds.tolist())
    for u, (name, _, _) in enumerate(cases):
        assert _record(r, u) == _expected(name), name
        assert rounds[u] >= 1, name
    for sub in ("0", "1"):
        os.environ["SSW_FPA_SUB"] = sub
        try:
            r2, rounds2 = _recognize(gpu_en, feats, plan, which)
        finally:
            del os.environ["SSW_FPA_SUB"]
        print("SSW_FPA_SUB=%s rounds per utterance:" % sub, rounds2.tolist())
        for u, (name, _, _) in enumerate(cases):
            assert _record(r2, u) == _expected(name), (sub, name)
            assert rounds2[u] >= 1, (sub, name)


def test_two_large_grammars_alternating_and_the_call_repeated(gpu_en):
    """per-utterance workspace, history and mask offsets; the second call finds the tables on the
    device"""
    plan = _plan(gpu_en, ["loop200", "loop400"])
    feats = _feats(gpu_en, 0)
    which = [0, 1] * 4
    r, rounds = _recognize(gpu_en, [feats] * 8, plan, which)
    print("rounds per utterance:", rounds.tolist())
    for u, g in enumerate(which):
        assert _record(r, u) == _expected(("loop200", "loop400")[g]), u
    r2, rounds2 = _recognize(gpu_en, [feats] * 8, plan, which)
    assert [_record(r2, u) for u in range(8)] == [_record(r, u) for u in range(8)]
    assert rounds2.tolist() == rounds.tolist()


def test_rounds_over_history_groups(gpu_en, monkeypatch):
    """loop400's history is 22.0 MB per utterance: under a 30 MB budget three of them are three
    groups, each round launches the unproven members of each group, and the groups share one
    table"""
    plan = _plan(gpu_en, ["loop400"])
    feats = _feats(gpu_en, 0)
    cut = _feats(gpu_en, 19200)
    monkeypatch.setenv("SSW_GRAMMAR_HIST_MB", "30")
    assert plan.history_groups([0, 278, 556, 834]) == 3
    r, rounds = _recognize(gpu_en, [feats] * 3, plan)
    print("rounds per utterance:", rounds.tolist())
    for u in range(3):
        assert _record(r, u) == _expected("loop400"), u
    # utterances that are proven in different rounds: a group without a member is skipped
    assert plan.history_groups([0, 278, 397, 675]) == 2
    r, rounds = _recognize(gpu_en, [feats, cut, feats], plan)
    print("rounds per utterance:", rounds.tolist())
    assert [_record(r, u) for u in range(3)] \
        == [_expected(n) for n in ("loop400", "loop400_1200ms", "loop400")]


def _flags2list(O, bits, n_sen):
    return O.flags2list(np.ascontiguousarray(bits, np.uint32), n_sen)


def test_rows_are_the_references_scores_and_close_the_loop(gpu_en, orc_en, oracle_mod):
    """loop200_1200ms with the rows and the listed senones returned: walking the frames in order,
    every listed senone's score is what the CPU oracle's restatement of ptm_mgau_frame_eval gives
    for that frame's list (compallsen = no) -- an export that listed too many HMMs would score
    other rows and could still land on the right words; and the plain grammar search over those
    rows, which reads only listed entries, gives the same record."""
    O = oracle_mod
    lex = _lex(gpu_en)
    feats = _feats(gpu_en, 19200)
    n = len(feats)
    plan = _plan(gpu_en, ["loop200"])
    d_rows = torch.zeros((n, gpu_en.n_sen), dtype=torch.int16, device="cuda")
    r, rounds, listed = _recognize(gpu_en, [feats], plan, d_senscr=d_rows, want_listed=True)
    torch.cuda.synchronize()
    print("rounds", rounds.tolist())
    assert _record(r, 0) == _expected("loop200_1200ms")
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


def test_recognize_audio_batch_active_on_a_large_grammar(gpu_en):
    """PCM in, the reference's JSON line out: active=True gives the default configuration's,
    active=False on the same flagged plan still the compallsen = yes one"""
    pcm = C.pcm("goforward.raw", 0)
    plan = _plan(gpu_en, ["loop200"])
    r = ssw.recognize_audio_batch(gpu_en, _lex(gpu_en), pcm, [0, len(pcm)], plan, active=True)
    assert r.json(0) == RESULTS["loop200"]["json"]
    assert r.hyp(0) == RESULTS["loop200"]["hyp"] and r.score(0) == RESULTS["loop200"]["score"]
    r = ssw.recognize_audio_batch(gpu_en, _lex(gpu_en), pcm, [0, len(pcm)], plan, active=False)
    assert r.json(0) == RESULTS_YES["loop200"]["json"]
    assert r.score(0) == RESULTS_YES["loop200"]["score"] != RESULTS["loop200"]["score"]


def test_a_flagged_plan_of_small_grammars_goes_through_the_one_workgroup_kernels(gpu_en):
    plan = _plan(gpu_en, ["goforward", "loop110"])
    feats = _feats(gpu_en, 0)
    assert plan.history_groups([0, 278, 556]) == 1
    r, rounds = _recognize(gpu_en, [feats] * 2, plan, [0, 1])
    print("rounds per utterance:", rounds.tolist())
    assert _record(r, 0) == _expected("goforward")
    assert _record(r, 1) == _expected("loop110")


def test_stats_grow_by_what_the_call_reported(gpu_en):
    feats = _feats(gpu_en, 0)
    cut = _feats(gpu_en, 19200)
    plan = _plan(gpu_en, ["loop200"])
    before = gpu_en.grammar_active_stats()
    fp_before = gpu_en.first_pass_active_stats()
    r, rounds = _recognize(gpu_en, [feats, cut, feats], plan)
    after = gpu_en.grammar_active_stats()
    assert after[0] - before[0] == 3
    assert after[1] - before[1] == int(rounds.sum())
    assert after[2] == int(rounds.max())
    assert after[3] - before[3] == int((rounds > 1).sum())
    assert gpu_en.first_pass_active_stats() == fp_before   # the first pass's counters are its own
    assert _record(r, 1) == _expected("loop200_1200ms")
