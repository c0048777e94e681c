"""Frame down-sampling (ssw_config_t.ds > 1, the reference's ds_ratio, src/ptm_mgau.c:241) at every
scoring entry point, bit-exact against the CPU oracle loaded with the same ds.

With ds > 1 a codebook is re-scanned only on the frames whose number WITHIN THE UTTERANCE is a
multiple of ds; the frames in between re-score the carried codewords.  Every frame then depends on
its predecessor and on its own frame number, and the PTM path leaves the speculative scans for
ptm_topn_chain_kernel (soundswallower_amd/csrc/ssw_k1a_chain.inc).  What can go wrong is the frame number a launch
counts from: a launch that starts in the middle of an utterance (a piece of ssw_score_batch_host's
cut, a continuation through carry_in, the vtable's one-frame launches) has to keep the utterance's
phase, and a launch that starts an utterance has to restart it.

Nothing is tolerated: int16 rows and, where the call exposes it, the top-N codeword order are
compared for equality.  One GPU model and one oracle per ds value for the whole module."""
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_alignment_task, synth_features
from tests import fsg_common as C
from tests.conftest import MODEL_ROOT, ROOT
from tests.test_cabi_host import synth_mixw_from_sendump
from tests.test_gpu_compact import _both_ways, _compact_rows, _task
from tests.test_gpu_dropin import _random_active_list
from tests.test_gpu_first_pass import _lex, _olex
from tests.test_gpu_grammar import _record
from tests.test_gpu_ptm import _oracle_batch, _ring_features, _tie_heavy_features
from tests.test_gpu_two_pass_history import _second_pass

pytestmark = pytest.mark.gpu
TEXT = "go forward ten meters".split()
SENTINEL = 0x5a5a


@pytest.fixture(scope="module")
def ds_models(oracle_mod):
    """get(d) -> (ssw.Model, oracle Model) of en-us with ds = d; loaded once per d"""
    mdir = ssw.model_dir("en-us")
    cache = {}

    def get(d):
        if d not in cache:
            cache[d] = (ssw.Model(mdir, config={"ds": d}), oracle_mod.Model(mdir, config={"ds": d}))
        return cache[d]
    yield get
    for g, _ in cache.values():
        g.close()


@pytest.fixture(scope="module")
def ds3_lex(ds_models):
    lex = _lex(ds_models(3)[0], "en-us")
    yield lex
    lex.free()


@pytest.fixture(scope="module")
def goforward_ds3(ds_models):
    """the reference's recording as the ds = 3 model's features, the ds = 3 oracle's rows of the
    first scoring and of the second one after the rewind (history carried, frame numbers restarted)"""
    g, o = ds_models(3)
    cep = np.load(os.path.join(ROOT, "tests", "golden", "goforward_mfcc.npy")).astype(np.float32)
    f39 = g.feat_batch(cep)
    rows1 = o.ptm_score_utt(f39)
    rows2 = o.ptm_score_chain(f39, [0, len(f39)], reset=False)
    return f39, rows1, rows2


# ---- 1. the host call's cut of a long utterance ------------------------------------------------
CUT_OFF = np.array([0, 10, 210, 210, 217], np.int32)


def _cut_batch(means):
    return np.concatenate([synth_features(means, 10, 4241), synth_features(means, 200, 4242),
                           synth_features(means, 7, 4243)])


@pytest.mark.parametrize("ds,cap", [(3, 64), (5, 64), (4, 66), (2, 64)])
def test_host_call_cut_keeps_the_utterance_phase(ds_models, means_en, monkeypatch, ds, cap):
    """ssw_score_batch_host cuts an utterance longer than SSW_HOST_PIPE_CAP into pieces, each a
    launch of its own.  A continuing piece must count its frames from its offset within the
    utterance: launched from 0 (as every piece was before ChainParams.frame_base was passed down)
    it re-scans on the wrong frames whenever ds does not divide the cap -- rows of the 200-frame
    utterance that differed then, counted with the oracle: (3, 64) 128, (5, 64) 136, (4, 66) 68;
    (2, 64) none, the cap being even.  One short utterance before the long one, an empty one and a
    7-frame one behind it (grouped, phase 0 each)."""
    g, o = ds_models(ds)
    feats = _cut_batch(means_en)
    ref, rcw, _ = _oracle_batch(o, feats, CUT_OFF[[0, 1, 2, 4]])    # (the empty one has no rows)
    # not a vacuous pass: pieces whose frame numbers restart are not the utterance
    long_ = feats[10:210]
    pieces = np.array(list(range(0, 200, cap)) + [200], np.int32)
    restarted = o.ptm_score_chain(long_, pieces)
    n_differ = int((restarted != ref[10:210]).any(axis=1).sum())
    print("ds %d cap %d: %d rows of 200 differ when the pieces restart the phase" % (ds, cap, n_differ))
    if cap % ds:
        assert n_differ >= 60
    else:
        assert n_differ == 0
    uncut = g.score_batch(feats, CUT_OFF)
    cw_uncut, _ = g.last_topn(len(feats))
    monkeypatch.setenv("SSW_HOST_PIPE_CAP", str(cap))
    cut = g.score_batch(feats, CUT_OFF)
    cw_cut, _ = g.last_topn(len(feats))
    monkeypatch.delenv("SSW_HOST_PIPE_CAP")
    bad = np.flatnonzero((cut != uncut).any(axis=1))
    print("rows of the cut call that differ from the uncut call: %d" % len(bad), bad[:8].tolist())
    assert np.array_equal(cut, uncut)
    assert np.array_equal(uncut, ref)
    assert np.array_equal(cut, ref)
    assert np.array_equal(cw_cut, cw_uncut)
    assert np.array_equal(cw_uncut.astype(np.int32), rcw)


def test_prescore_of_a_cut_utterance(ds_models, means_en, monkeypatch):
    """ssw_mgau_prescore goes through the same call: the cached rows at, around and far from the
    piece edges (ds = 3, pieces of 64)"""
    g, o = ds_models(3)
    feats = synth_features(means_en, 200, 4242)
    ref = o.ptm_score_utt(feats)
    mg = ssw.PtmMgau(g)
    monkeypatch.setenv("SSW_HOST_PIPE_CAP", "64")
    try:
        mg.prescore(feats)
        for t in (0, 63, 64, 65, 199):
            assert np.array_equal(mg.frame_eval(feats[t], t), ref[t]), t
    finally:
        mg.free()


# ---- 2. an utterance continued by a second call; the ring over utterances ----------------------
def test_two_calls_continue_an_utterance_at_a_multiple_of_lcm_2_ds(ds_models, means_en):
    """include/ssw_amd.h, carry_out: ssw_score_batch_ex numbers every utterance of a call from 0,
    so a continuation is the reference's scoring when the first call ends after a multiple of
    lcm(2, ds) frames: 66 of 150 at ds = 3.  Plain frames and runs of tied frames (where the order
    carried in decides)."""
    g, o = ds_models(3)
    for feats in (synth_features(means_en, 150, 808), _tie_heavy_features(o, means_en, 150, 7)):
        ref = o.ptm_score_utt(feats)
        a, carry = g.score_batch_carry(feats[:66])
        b, _ = g.score_batch_carry(feats[66:], carry_in=carry)
        assert np.array_equal(np.concatenate([a, b]), ref)


def test_chain_over_utterances_at_ds3(ds_models, means_en):
    """SSW_SCORE_CARRY_UTTS at ds = 3: frame numbers -- the ds phase and the two-slot ring -- restart
    with every utterance (odd cuts are not phase-aligned here, as they all are at ds = 2).  One
    call, and two calls split at utterance boundaries with SSW_SCORE_CARRY_OUT_REWIND."""
    g, o = ds_models(3)
    feats, off = _ring_features(o, means_en, 300)
    want = o.ptm_score_chain(feats, off)
    got, _ = g.score_batch_carry(feats, off, carry_utts=True)
    assert np.array_equal(got, want)
    for cut_u in (1, 2, 3, 4, 6, 9):     # behind utterances of 3, 4, 1, 0, 5 frames, and later
        cut = int(off[cut_u])
        a, carry = g.score_batch_carry(feats[:cut], off[:cut_u + 1], carry_utts=True, rewind=True)
        b, _ = g.score_batch_carry(feats[cut:], off[cut_u:] - cut, carry_in=carry, carry_utts=True)
        assert np.array_equal(np.concatenate([a, b]), want), cut_u


# ---- 3. the vtable, frame by frame -------------------------------------------------------------
def _frame_lists(oracle_mod, o, n, seed):
    """active lists as tests/test_gpu_dropin.py::test_mgau_vtable_compallsen_no builds them"""
    rng = np.random.default_rng(seed)
    lists = []
    for t in range(n):
        lst = _random_active_list(oracle_mod, o.n_sen, rng, (0.002, 0.02, 0.3, 1.0)[t % 4])
        lists.append(lst[:0] if t == 5 else lst)             # nothing active at all
    return lists, _random_active_list(oracle_mod, o.n_sen, rng, 0.1)


def _n_active_codebooks(o, lst):
    sens = np.cumsum(np.asarray(lst, np.int64))
    return len(np.unique(np.asarray(o.sen2cimap)[sens]))


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "active_lists"])
@pytest.mark.parametrize("ds", [2, 3])
def test_vtable_frame_by_frame(ds_models, oracle_mod, means_en, ds, active):
    """ptm_mgau_frame_eval driven as acmod drives it on a ds model: frame_idx written from outside,
    two utterances (9 and 10 frames) without a reset in between, a past frame re-scored, then the
    second utterance once more from frame_idx = 0 as decoder_alignment does after its rewind (the
    phase restarts, frame 0 copies slot 1).  With active lists some codebooks are inactive on
    frames that are scanned (frame % ds == 0)."""
    g, o = ds_models(ds)
    mg = ssw.PtmMgau(g)
    o.ptm_reset()
    utts = [synth_features(means_en, 9, 500), synth_features(means_en, 10, 501)]
    lists, relist = _frame_lists(oracle_mod, o, 10, 5) if active else (None, None)
    if active:
        assert any(t % ds == 0 and 0 < _n_active_codebooks(o, lists[t]) < o.n_cb for t in range(9))

    def both(feat, t, lst):
        if lst is None:
            return mg.frame_eval(feat, t), o.ptm_frame_eval(feat, t)
        return (mg.frame_eval(feat, t, compallsen=False, senone_active=lst),
                o.ptm_frame_eval(feat, t, compallsen=False, senone_active=lst))

    def run(feats, tag):
        mg.frame_idx = 0
        o.ptm_set_frame_idx(0)
        for t in range(len(feats)):
            got, ref = both(feats[t], t, lists[t] if active else None)
            assert np.array_equal(got, ref), (tag, t)
            if t == 4:                        # a past frame: the stored top-N, the features ignored
                mg.frame_idx = t + 1
                o.ptm_set_frame_idx(t + 1)
                again, ref2 = both(np.zeros(39, np.float32) if not active else feats[t], t,
                                   relist if active else None)
                assert np.array_equal(again, ref2), (tag, t, "again")
                if not active:
                    assert np.array_equal(again, ref)
            mg.frame_idx = t + 1              # acmod_advance
            o.ptm_set_frame_idx(t + 1)
    try:
        run(utts[0], "first")
        run(utts[1], "second")
        run(utts[1], "second, after the rewind")
    finally:
        mg.free()


# ---- 4. compact rows ---------------------------------------------------------------------------
def test_compact_rows_at_ds3(ds_models, means_en):
    """ssw_score_batch_compact on a ds = 3 model: every state's column holds the oracle's score of
    its senone; and the compact pipeline equals the full-row one (tests/test_gpu_compact.py)."""
    g, o = ds_models(3)
    feats, frame_off, phone_off, senid, tmat = _task(g, o, means_en, [60, 61, 59], [10, 12, 9], 3100)
    full, _, _ = _oracle_batch(o, feats, frame_off)
    plan = g.compact_plan(frame_off, phone_off, senid)
    d_feats = g.to_device(feats)
    d_c = g.device_malloc(max(plan.nbytes, 2))
    try:
        g.score_batch_compact(d_feats, plan, d_c)
        g._L.ssw_device_synchronize()
        rows = _compact_rows(g, plan, d_c, frame_off, phone_off)
    finally:
        g.device_free(d_feats)
        g.device_free(d_c)
        plan.free()
    sen = np.asarray(senid, np.uint16).reshape(-1)
    for u, r in enumerate(rows):
        ids = sen[phone_off[u] * 3:phone_off[u + 1] * 3].astype(np.int64)
        uniq, first = np.unique(ids, return_index=True)      # a senone's score sits at its first state
        assert r.shape[0] == frame_off[u + 1] - frame_off[u]
        assert np.array_equal(r[:, first], full[frame_off[u]:frame_off[u + 1]][:, uniq]), u
    _both_ways(g, feats, frame_off, phone_off, senid, tmat)


# ---- 5. flows that consume the scores ----------------------------------------------------------
@pytest.mark.parametrize("history", [0, 1])
def test_align_text_batch_at_ds3(ds_models, ds3_lex, goforward_ds3, oracle_mod, history):
    """ssw_align_text_batch on a ds = 3 model, the reference's recording twice in one batch: the
    words are the oracle's first pass over the ds = 3 oracle's rows, the state alignment the second
    pass over the same rows (two_pass_history = 0) or over the rows of the second scoring after
    the rewind (two_pass_history = 1: history carried, frame numbers -- the phase -- restarted)."""
    g, o = ds_models(3)
    f39, rows1, rows2 = goforward_ds3
    n = len(f39)
    F, olex = _olex(oracle_mod, o, "en-us")
    want_seg = F.first_pass(o, olex, TEXT, rows1)
    assert want_seg is not None
    want_words, want_st = _second_pass(g, ds3_lex, rows1, rows2 if history else rows1, n)
    assert want_words == [w for (w, _, _, _) in want_seg]
    print("rows that differ between the two scorings:", int((rows1 != rows2).any(axis=1).sum()))
    d_feats = torch.from_numpy(np.concatenate([f39, f39])).cuda()
    cfg = ds3_lex.first_pass_config(two_pass_history=history)
    aset = ssw.align_text_batch(g, ds3_lex, d_feats, [0, n, 2 * n], [TEXT] * 2, cfg=cfg)
    try:
        for u in range(2):
            assert aset.status(u) == 0, u
            got = aset.utterance(u)
            assert [(w, int(e[0]), int(e[0]) + int(e[1]) - 1)
                    for w, e in zip(got["words"], got["word_al"])] \
                == [(w, s, e) for (w, s, e, _) in want_seg], u
            assert np.array_equal(got["state_al"], want_st), u
    finally:
        aset.free()


def test_recognize_batch_at_ds3(ds_models, ds3_lex, goforward_ds3, oracle_mod):
    """ssw_recognize_batch on a ds = 3 model against tests/golden/fsg/goforward.fsg: the record is
    the grammar search's over the ds = 3 oracle's rows; and, oracle/fsg_oracle.py restating the
    search of linear grammars only, the text's chain grammar through the same call gives the
    oracle's first pass over those rows (as tests/test_gpu_grammar.py compares them)."""
    g, o = ds_models(3)
    f39, rows1, _ = goforward_ds3
    n = len(f39)
    off = np.array([0, n], np.int32)
    d_feats = torch.from_numpy(f39).cuda()
    d_rows = torch.from_numpy(rows1).cuda()
    plan = ds3_lex.grammar_plan(ssw.Fsg.read(g, ds3_lex, C.fsg_path("goforward")))
    r = ssw.recognize_batch(g, ds3_lex, d_feats, off, plan)
    want = ssw.grammar_search_batch(g, ds3_lex, d_rows, off, plan)
    print(_record(r, 0))
    assert _record(r, 0) == _record(want, 0)
    F, olex = _olex(oracle_mod, o, "en-us")
    seg = F.first_pass(o, olex, TEXT, rows1)
    assert seg is not None
    chain = ssw.Fsg.create(g, ds3_lex, "chain", 0, len(TEXT),
                           [(i, i + 1, 1.0, w) for i, w in enumerate(TEXT)])
    rc = ssw.recognize_batch(g, ds3_lex, d_feats, off, ds3_lex.grammar_plan(chain))
    assert rc.status(0) == 0
    got, total = [], 0
    for w, sf, ef, ascr, lscr in rc.segments(0):
        total += ascr + lscr
        got.append((w, sf, ef, total))
    assert got == seg
    assert rc.score(0) == seg[-1][3]


# ---- 6. what is refused stays refused, and early -----------------------------------------------
def test_active_set_batches_are_refused_before_anything_runs(ds_models, means_en):
    """ds = 2: the batched active-set calls serve ds = 1 only and say so before a launch; the
    caller's score rows still hold what they held."""
    g, o = ds_models(2)
    n_fr, n_ph = 30, 5
    feats = synth_features(means_en, n_fr, 66)
    senid, tmat, _ = synth_alignment_task(o.sseq, o.phone_ssid, o.phone_tmat, o.n_ciphone, n_ph, 66)
    mark = np.full((n_fr, g.n_sen), SENTINEL, np.int16)
    d_feats = g.to_device(feats)
    d_scr = g.to_device(mark)
    back = np.zeros_like(mark)
    try:
        with pytest.raises(ssw.SswError, match="active-set batches: ds = 1 only"):
            g.align_batch_active(d_feats, [0, n_fr], [0, n_ph], senid, tmat, d_senscr=d_scr)
        g._L.ssw_device_synchronize()
        g._L.ssw_memcpy_d2h(back.ctypes.data, d_scr, back.nbytes)
    finally:
        g.device_free(d_feats)
        g.device_free(d_scr)
    assert np.array_equal(back, mark)
    lex = _lex(g, "en-us")
    message = r"frame down-sampling \(ds != 1\) is served by the per-frame calls only"
    t_feats = torch.from_numpy(feats).cuda()
    t_rows = torch.full((n_fr, g.n_sen), SENTINEL, dtype=torch.int16, device="cuda")
    before = g.first_pass_active_stats()
    try:
        with pytest.raises(ssw.SswError, match=message):
            lex.first_pass_active(t_feats, [0, n_fr], [TEXT], d_senscr=t_rows)
        with pytest.raises(ssw.SswError, match=message):
            ssw.align_text_batch_active(g, lex, t_feats, [0, n_fr], [TEXT])
    finally:
        lex.free()
    torch.cuda.synchronize()
    assert bool((t_rows == SENTINEL).all())
    assert g.first_pass_active_stats() == before


# ---- 7. the ms scorer has no ds ----------------------------------------------------------------
def test_ms_scorer_reads_no_ds(oracle_mod, orc_fr, means_fr, tmp_path):
    """only ptm_mgau.c (and s2_semi_mgau.c) read ds in the reference: a model loaded with ds = 3
    scores through SSW_SCORER_MS what a ds = 1 oracle's ms scorer gives"""
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    g = ssw.Model(variances=os.path.join(src, "variances"), config={"ds": 3}, **kw)
    o = oracle_mod.Model(vars=os.path.join(src, "variances"), **kw)
    try:
        feats = synth_features(means_fr, 40, 2468)
        got = g.score_batch(feats, scorer=ssw.SCORER_MS)
        assert np.array_equal(got, o.ms_score_utt(feats))
    finally:
        g.close()
