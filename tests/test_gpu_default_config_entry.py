"""The host entry of the default configuration's loop of speculation and proof
(csrc/ssw_host_fpactive.inc, its grammar callers in csrc/ssw_host_grammar.inc): one request per
call, the round policy, the workspace laid out once per call, the four *_active entry points'
shared s2_semi route and their own orders of refusals.

Every case LOADS ITS OWN model (the session-wide ones have whatever an earlier test left in
their workspaces and caches) and compares bit for bit with the same call on a freshly loaded
one.  Features are cut from tests/golden/goforward_mfcc.npy; what a cut utterance aligns or
recognises to does not matter here, only that it is what a fresh model gives -- and that the
loop is entered: the cuts are ones of which at least one utterance needs more than one round."""
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fsg_common as FC
from tests.conftest import MODEL_ROOT
from tests.test_gpu_workspace_growth import Ctx, _aset_record, _batch, _rset_record, f39  # noqa: F401

pytestmark = pytest.mark.gpu

TEXTS3 = [["go"], ["go", "forward"], ["go", "forward", "ten"]]
LENS3 = [24, 40, 60]
TEXTS6 = TEXTS3 + [["forward"], ["go", "forward"], ["ten"]]
LENS6 = [24, 40, 60, 30, 36, 52]
# every utterance from frame 140 on: "go forward ten meters" is over by then, and of these cuts
# the second, third and fifth take four rounds against TEXTS3 / TEXTS6, all six two to four
# against WHOLE (and against goforward.fsg): the second round is then over the whole batch
# again, the third over five utterances as a subset, the fourth over four, one by one
START = 140
WHOLE = [["go", "forward", "ten", "meters"]] * 6


def _fresh(run, **kw):
    c = Ctx(**kw)
    try:
        return run(c)
    finally:
        c.close()


def _first_pass(c, f39, lens, texts, cfg=None):
    """ssw_first_pass_batch_active: segmentations, rounds, the seed and the whole rows"""
    feats, off = _batch(f39, lens, start=START)
    d = c.m.to_device(feats)
    d_rows = torch.zeros((int(off[-1]), c.m.n_sen), dtype=torch.int16, device="cuda")
    try:
        segs, rounds, seed = c.lex.first_pass_active(d, off, texts, cfg=cfg, d_senscr=d_rows, want_seed=True)
        torch.cuda.synchronize()
        return segs, rounds.tolist(), seed.tobytes(), d_rows.cpu().numpy().tobytes()
    finally:
        c.m.device_free(d)


def _align_text(c, f39, lens, texts, two_pass):
    """ssw_align_text_batch_active, and with two_pass_history the orders it carried"""
    feats, off = _batch(f39, lens, start=START)
    d = c.m.to_device(feats)
    try:
        cfg = c.lex.first_pass_config(two_pass_history=two_pass)
        rec = _aset_record(ssw.align_text_batch_active(c.m, c.lex, d, off, texts, cfg=cfg), len(lens))
        carry = c.m.first_pass_active_carry(len(lens)).tobytes() if two_pass else None
        return rec, carry, c.m.first_pass_active_stats()[2]
    finally:
        c.m.device_free(d)


def _goforward(c):
    if not c.plans:
        c.fsgs["g"] = ssw.Fsg.read(c.m, c.lex, FC.fsg_path("goforward"))
        c.plans["g"] = c.lex.grammar_plan(c.fsgs["g"])
    return c.plans["g"]


@pytest.mark.parametrize("sub", [None, "0", "1"])
def test_round_policy(f39, monkeypatch, sub):
    """SSW_FPA_SUB unset (the unproven utterances one by one once they are few), 0 (always the
    whole batch) and 1 (always one by one): the same segmentations, rounds, seed and rows as one
    another -- each against the unset call on a fresh model -- over six utterances (the
    whole-batch rule needs more than four) of which some need more than one round."""
    def run(c):
        return _first_pass(c, f39, LENS6, WHOLE)

    want = _fresh(run)
    if sub is not None:
        monkeypatch.setenv("SSW_FPA_SUB", sub)
    got = _fresh(run)
    print("SSW_FPA_SUB=%s rounds per utterance:" % sub, got[1])
    assert got == want
    assert min(got[1]) > 1 and max(got[1]) > 3


def test_workspace_reuse(f39):
    """Six utterances, three, the six again on one model; the calls in between with and without
    two-pass history, which alone lays out the utterance-start words behind everything else."""
    def six(c):
        return _first_pass(c, f39, LENS6, TEXTS6)

    def three(c):
        return _first_pass(c, f39, LENS3, TEXTS3)

    def carried(c):
        return _align_text(c, f39, LENS6, TEXTS6, 1)

    def plain(c):
        return _align_text(c, f39, LENS3, TEXTS3, 0)

    c = Ctx()
    try:
        got = [six(c), carried(c), three(c), plain(c), six(c), carried(c)]
    finally:
        c.close()
    want = [_fresh(six), _fresh(carried), _fresh(three), _fresh(plain)]
    assert got == want + want[:2]
    assert max(want[0][1]) > 1 and want[1][2] > 1
    assert want[1][1] is not None and want[3][1] is None


def test_recognize_batch_active_with_listed_and_rows(f39):
    """ssw_recognize_batch_active with `listed` and d_senscr: hypotheses, rounds, the listed
    senones of every frame and the whole rows, after another call on the same model"""
    def run(c, lens=LENS6):
        feats, off = _batch(f39, lens, start=START)
        d = c.m.to_device(feats)
        d_rows = torch.zeros((int(off[-1]), c.m.n_sen), dtype=torch.int16, device="cuda")
        try:
            r, rounds, listed = ssw.recognize_batch_active(c.m, c.lex, d, off, _goforward(c),
                                                           d_senscr=d_rows, want_listed=True)
            torch.cuda.synchronize()
            return _rset_record(r), rounds.tolist(), listed.tobytes(), d_rows.cpu().numpy().tobytes()
        finally:
            c.m.device_free(d)

    c = Ctx()
    try:
        run(c, LENS3)
        got = run(c)
    finally:
        c.close()
    print("rounds per utterance:", got[1])
    assert got == _fresh(run)
    assert max(got[1]) > 1
    assert np.frombuffer(got[2], np.uint32).any()


@pytest.mark.parametrize("two_pass", [False, True])
def test_recognize_align_batch_active(f39, two_pass):
    """ssw_recognize_align_batch_active without and with two_pass_history (the carried orders
    come from the loop), after another call on the same model"""
    def run(c, lens=LENS6):
        feats, off = _batch(f39, lens, start=START)
        d = c.m.to_device(feats)
        try:
            r, a, rounds = ssw.recognize_align_batch_active(c.m, c.lex, d, off, _goforward(c),
                                                            two_pass_history=two_pass)
            return _rset_record(r), _aset_record(a, len(lens)), rounds.tolist()
        finally:
            c.m.device_free(d)

    c = Ctx()
    try:
        run(c, LENS3)
        got = run(c)
    finally:
        c.close()
    print("rounds per utterance:", got[2])
    assert got == _fresh(run)
    assert max(got[2]) > 1


def test_zero_frame_inputs(f39):
    """An utterance of no frames inside a batch, and a batch of no utterances, through every
    entry"""
    lens = [24, 0, 60, 30, 0, 52]

    def run(c):
        out = [_first_pass(c, f39, lens, TEXTS6), _align_text(c, f39, lens, TEXTS6, 1)]
        feats, off = _batch(f39, lens, start=START)
        d = c.m.to_device(feats)
        try:
            r, rounds = ssw.recognize_batch_active(c.m, c.lex, d, off, _goforward(c))
            out.append((_rset_record(r), rounds.tolist()))
            r, a, rounds = ssw.recognize_align_batch_active(c.m, c.lex, d, off, _goforward(c),
                                                            two_pass_history=True)
            out.append((_rset_record(r), _aset_record(a, len(lens)), rounds.tolist()))
            # no utterance at all
            none = np.zeros(1, np.int32)
            stats = c.m.first_pass_active_stats(), c.m.grammar_active_stats()
            assert c.lex.first_pass_active_raw(d, none, [])[0].size == 0
            ssw.align_text_batch_active(c.m, c.lex, d, none, []).free()
            r, rounds = ssw.recognize_batch_active(c.m, c.lex, d, none, _goforward(c))
            assert len(r) == 0 and rounds.size == 0
            r.free()
            r, a, rounds = ssw.recognize_align_batch_active(c.m, c.lex, d, none, _goforward(c))
            r.free()
            a.free()
            assert stats == (c.m.first_pass_active_stats(), c.m.grammar_active_stats())
        finally:
            c.m.device_free(d)
        return out

    got = _fresh(run)
    assert got == _fresh(run)
    assert got[0][0][1] is None and got[0][0][4] is None
    assert max(got[0][1]) > 1 or max(got[2][1]) > 1


def test_s2_semi_refusals(f39):
    """The s2_semi scorer makes no sets of listed senones: seed_active and listed are refused,
    each by its message, before anything is scored"""
    c = Ctx()
    feats, off = _batch(f39, LENS3, start=START)
    d = c.m.to_device(feats)
    try:
        with pytest.raises(ssw.SswError) as e:
            c.lex.first_pass_active(d, off, TEXTS3, scorer=ssw.SCORER_S2_SEMI, want_seed=True)
        assert ("ssw_first_pass_batch_active: the s2_semi scorer makes no sets of listed senones "
                "(seed_active)") in str(e.value)
        with pytest.raises(ssw.SswError) as e:
            ssw.recognize_batch_active(c.m, c.lex, d, off, _goforward(c), scorer=ssw.SCORER_S2_SEMI,
                                       want_listed=True)
        assert ("ssw_recognize_batch_active: the s2_semi scorer makes no sets of listed senones "
                "(listed)") in str(e.value)
        assert c.m.first_pass_active_stats() == (0, 0, 0, 0) == c.m.grammar_active_stats()
    finally:
        c.m.device_free(d)
        c.close()


def test_refusal_order():
    """One call with two faults per entry; the message that wins is the one that won before the
    entries shared their helpers.  The model is loaded with ds = 2, which the loop refuses."""
    mdir = os.path.join(MODEL_ROOT, "en-us")
    m = ssw.Model(mdir, config={"ds": 2})
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    fsg = ssw.Fsg.read(m, lex, FC.fsg_path("goforward"))
    plan = lex.grammar_plan(fsg)
    off = np.array([0, 24, 64], np.int32)
    d = m.to_device(np.zeros((64, 39), np.float32))
    won = []

    def refused(call):
        with pytest.raises(ssw.SswError) as e:
            call()
        won.append(str(e.value))
        print(won[-1])
        return won[-1]

    try:
        # a word the dictionary does not have (the graphs are built first) + ds = 2
        assert "ssw_first_pass_batch_active: Unknown word xyzzy" in refused(
            lambda: lex.first_pass_active(d, off, [["go"], ["xyzzy"]]))
        # the s2_semi scorer on a model of many codebooks (its route scores first) + ds = 2
        assert "ssw_align_text_batch_active: s2_semi scorer: the model has 42 codebooks, not one" in refused(
            lambda: ssw.align_text_batch_active(m, lex, d, off, [["go"], ["forward"]],
                                                scorer=ssw.SCORER_S2_SEMI))
        # `listed` with the s2_semi scorer (refused before its route scores) + many codebooks
        assert "makes no sets of listed senones (listed)" in refused(
            lambda: ssw.recognize_batch_active(m, lex, d, off, plan, scorer=ssw.SCORER_S2_SEMI,
                                               want_listed=True))
        # ds = 2 (refused before the run begins) + a grammar index beyond the plan
        assert "ssw_recognize_align_batch_active: frame down-sampling (ds != 1)" in refused(
            lambda: ssw.recognize_align_batch_active(m, lex, d, off, plan, fsg_of_utt=[0, 7]))
    finally:
        m.device_free(d)
        plan.free()
        fsg.free()
        lex.free()
        m.close()
