"""The host entry of the first pass and of decoder_alignment's second half
(csrc/ssw_host_firstpass.inc): one request per run, the export of the active sets an argument of
it, the cached-graphs policy, the three ways a run's results come back, the timing lines.

Every case LOADS ITS OWN model (the session-wide ones have whatever an earlier test left in
their workspaces and caches) and compares bit for bit with the same call on a freshly loaded
one.  Features are cut from tests/golden/goforward_mfcc.npy; what a cut utterance aligns to
does not matter here, only that it is what a fresh model gives."""
import re

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import lcg_uniform
from tests.test_gpu_first_pass import _olex, synth_scores
from tests.test_gpu_workspace_growth import Ctx, _aset_record, _batch, f39  # noqa: F401

pytestmark = pytest.mark.gpu

TEXTS = [["go"], ["go", "forward"], ["go", "forward", "ten"]]
LENS_A, LENS_B = [24, 40, 60], [30, 36, 52]


def _planned(c, plan, f39, lens, start):
    """forced_align_planned of `plan` over the scores of a cut of the recording"""
    feats, off = _batch(f39, lens, start=start)
    d = c.m.to_device(c.m.score_batch(feats, off))
    try:
        return _aset_record(ssw.forced_align_planned(c.m, c.lex, plan, d, off), len(lens))
    finally:
        c.m.device_free(d)


def _active(c, f39, lens, start):
    feats, off = _batch(f39, lens, start=start)
    d = c.m.to_device(feats)
    try:
        return _aset_record(ssw.align_text_batch_active(c.m, c.lex, d, off, TEXTS), len(lens))
    finally:
        c.m.device_free(d)


def _on_a_fresh_model(run):
    c = Ctx()
    try:
        return run(c)
    finally:
        c.close()


@pytest.mark.parametrize("kernel", [None, "big"])
def test_export_is_an_argument_of_the_run(f39, monkeypatch, kernel):
    """A plain search, a default-configuration one (its searches export the sets of active HMMs),
    a plain one again on the same model: the export of the second leaves nothing behind for the
    third.  SSW_FP_KERNEL=big: the long-text kernels' export path (the mask cleared first), its
    rounds on the cached graphs."""
    if kernel:
        monkeypatch.setenv("SSW_FP_KERNEL", kernel)

    def planned(c):
        plan = ssw.FirstPassPlan(c.m, c.lex, TEXTS)
        try:
            return _planned(c, plan, f39, LENS_A, 40)
        finally:
            plan.free()

    c = Ctx()
    try:
        first = planned(c)
        active = _active(c, f39, LENS_A, 40)
        third = planned(c)
    finally:
        c.close()
    assert first == third
    assert first == _on_a_fresh_model(planned)
    assert active == _on_a_fresh_model(lambda b: _active(b, f39, LENS_A, 40))
    assert any(r[0] == 0 for r in first) and any(r[0] == 0 for r in active)


@pytest.fixture(scope="module")
def short_and_long(oracle_mod, orc_en):
    """eighteen texts, one word and eight words in turn, with scores that follow each text"""
    F, olex = _olex(oracle_mod, orc_en, "en-us")
    vocab = [w for w in olex.order[:olex.filler_start] if "(" not in w]
    u = lcg_uniform(23, 18 * 10)
    texts, scores = [], []
    for t in range(18):
        n = 1 if t % 2 == 0 else 8
        texts.append([vocab[int(x * len(vocab))] for x in u[t * 10 + 1:t * 10 + 1 + n]])
        scores.append(synth_scores(F, orc_en, olex, texts[-1], 500 + t, orc_en.n_sen))
    return texts, scores


@pytest.mark.parametrize("n_texts", [6, 18])
def test_leftover_rows_come_back_in_both_regimes(short_and_long, monkeypatch, n_texts):
    """SSW_FP_KERNEL=big SSW_FP_HIST_BAND=6: the eight-word texts outgrow the history budget and
    are searched again one level down, they alone.  Three of them (of six texts): their rows are
    fetched one by one; nine (of eighteen): one copy of everything, picked on the host.  Every
    segmentation equals the unforced call's."""
    texts, scores = short_and_long[0][:n_texts], short_and_long[1][:n_texts]
    off = np.concatenate([[0], np.cumsum([len(s) for s in scores])]).astype(np.int32)
    c = Ctx()
    d = c.m.to_device(np.ascontiguousarray(np.concatenate(scores), np.int16))
    try:
        plain = c.lex.first_pass(d, off, texts)
        monkeypatch.setenv("SSW_FP_KERNEL", "big")
        monkeypatch.setenv("SSW_FP_HIST_BAND", "6")
        forced = c.lex.first_pass(d, off, texts)
    finally:
        c.m.device_free(d)
        c.close()
    assert forced == plain
    assert sum(g is not None for g in plain) >= n_texts - 2


def test_a_plan_meets_new_recordings_on_cached_graphs(f39):
    """One plan on a recording (its graphs go up), on another with other utterance lengths (the
    graphs are on the device: only the call's own tables go up, the utterance offsets and the
    history offsets ahead of the graph's among them), and on the first again."""
    def run(c, lens, start):
        if "p" not in c.plans:
            c.plans["p"] = ssw.FirstPassPlan(c.m, c.lex, TEXTS)
        return _planned(c, c.plans["p"], f39, lens, start)

    c = Ctx()
    try:
        got = [run(c, LENS_A, 40), run(c, LENS_B, 38), run(c, LENS_A, 40)]
    finally:
        c.close()
    fresh_a = _on_a_fresh_model(lambda b: run(b, LENS_A, 40))
    fresh_b = _on_a_fresh_model(lambda b: run(b, LENS_B, 38))
    assert got == [fresh_a, fresh_b, fresh_a]
    assert fresh_a != fresh_b


FP_LINE = re.compile(r"^ssw_first_pass_batch: graphs \d+\.\d\d ms \(\d+ HMMs\), "
                     r"upload \+ search \+ results \d+\.\d\d ms$")
AL_LINE = re.compile(r"^ssw_forced_align_batch: first pass \d+\.\d\d ms, populate \d+\.\d\d, "
                     r"second pass \d+\.\d\d, propagate \d+\.\d\d$")


def test_timing_lines(f39, short_and_long, monkeypatch, capfd):
    """SSW_ALIGN_TIMING=1: one forced_align_batch prints one ssw_first_pass_batch line per level
    run and one ssw_forced_align_batch line, in the present formats.  Short texts are searched
    in one run; the short and long ones under a history budget of 6 in two or three (the window
    level, then the HBM levels for what it left)."""
    monkeypatch.setenv("SSW_ALIGN_TIMING", "1")
    c = Ctx()
    try:
        feats, off = _batch(f39, LENS_A)
        d = c.m.to_device(c.m.score_batch(feats, off))
        capfd.readouterr()
        ssw.forced_align_batch(c.m, c.lex, d, off, TEXTS).free()
        short = capfd.readouterr().err.splitlines()
        c.m.device_free(d)
        texts, scores = short_and_long[0][:6], short_and_long[1][:6]
        off = np.concatenate([[0], np.cumsum([len(s) for s in scores])]).astype(np.int32)
        d = c.m.to_device(np.ascontiguousarray(np.concatenate(scores), np.int16))
        monkeypatch.setenv("SSW_FP_KERNEL", "big")
        monkeypatch.setenv("SSW_FP_HIST_BAND", "6")
        capfd.readouterr()
        ssw.forced_align_batch(c.m, c.lex, d, off, texts).free()
        levels = capfd.readouterr().err.splitlines()
        c.m.device_free(d)
    finally:
        c.close()
    for lines, n_runs in ((short, (1,)), (levels, (2, 3))):
        fp = [ln for ln in lines if ln.startswith("ssw_first_pass_batch:")]
        al = [ln for ln in lines if ln.startswith("ssw_forced_align_batch:")]
        assert len(fp) in n_runs and len(al) == 1, lines
        assert all(FP_LINE.match(ln) for ln in fp) and AL_LINE.match(al[0]), lines
        assert lines.index(al[0]) > lines.index(fp[-1])
        # every run of one call searches the same graphs
        assert len({re.search(r"\((\d+) HMMs\)", ln).group(1) for ln in fp}) == 1
