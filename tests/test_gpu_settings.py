"""Scoring, text alignment and recognition with logbase, varfloor, mixwfloor and tmatfloor away
from their defaults, on the GPU.

Every comparison is for equality: int16 rows and, where the call exposes it, the top-N codewords,
against the CPU oracle loaded with the same settings (tests/test_settings_host.py holds the
oracle's rows and tables to what the reference library recorded) and, for the reference's
recording, against those records themselves (tests/golden/settings_results.json).

What logbase moves in the kernels: the 8-bit log-add table's largest entry T and its reach decide
the folded table of ptm_senone_kernel (at 1.000018 it is at its limit: Hb = 255, 255 + 96 + 3 T =
465 of 512), whether the ms scorer takes the packed kernel (255 + 640 + 6 T < 1024) and how often
its frames are marked; the size of a score unit against float error moves the scans' exact-pass
lists (at 1.000018 the vector-unit scan leaves nearly every density to the exact form) and, at
1.003, makes scores tie everywhere.  One GPU model and one oracle per setting for the module;
the oracle's rows once per batch."""
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_features
from tests import cont_common as CC
from tests import mllr_common as M
from tests import sc_common as S
from tests import settings_common as SC
from tests.test_gpu_first_pass import _olex
from tests.test_gpu_grammar import _record
from tests.test_gpu_ptm import _oracle_batch
from tests.test_gpu_senone_fold import BATCHES, _batch, _extreme_features, _extreme_weights, _set
from tests.test_gpu_two_pass_history import _second_pass

pytestmark = pytest.mark.gpu

PTM_BASES = (1.000018, 1.00003, 1.0003, 1.001, 1.003)
KNOBS = {"default": {}, "generic": {"SSW_SEN_GENERIC": "1"}, "fma": {"SSW_SCAN": "fma"}}
MS_PICK = np.r_[0:96, 1020:1030, 2045:2049]
_REF = {}


def _once(key, make):
    if key not in _REF:
        v = make()
        for a in (v if isinstance(v, tuple) else (v,)):
            a.setflags(write=False)
        _REF[key] = v
    return _REF[key]


@pytest.fixture(scope="module")
def fx():
    return SC.results()


@pytest.fixture(scope="module")
def fr_dir(orc_fr, tmp_path_factory):
    return SC.fr_mixw_dir(str(tmp_path_factory.mktemp("settings_gpu") / "fr-mixw"), orc_fr)


@pytest.fixture(scope="module")
def models(oracle_mod, fr_dir):
    """get(model, settings) -> (ssw.Model on the GPU, oracle Model); loaded once per setting"""
    cache = {}

    def get(model, over):
        key = (model, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = (SC.load(model, over, None, fr_dir), SC.load_oracle(model, over, fr_dir))
        return cache[key]
    yield get
    for g, _ in cache.values():
        g.close()


def _same(got, ref):
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, bad[:8].tolist()


# ---------------------------------------------------------------------------------------------
# PTM under logbase
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", list(KNOBS))
@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("base", PTM_BASES)
def test_ptm_under_logbase(models, means_en, monkeypatch, base, batch, knobs):
    """the two instances of ptm_senone_kernel (2,049 frames: two per group, an odd last unit; 130:
    one per group), utterance starts inside the batch; the matrix-core scan, the vector-unit one
    (SSW_SCAN=fma) and the senone kernel's generic instance"""
    _set(monkeypatch, KNOBS[knobs])
    g, o = models("en-us", {"logbase": base})
    feats, off = _batch(means_en, BATCHES[batch], 6100)
    ref, rcw, _ = _once(("ptm", base, batch), lambda: _oracle_batch(o, feats, off))
    got = g.score_batch(feats, off)
    gcw, _ = g.last_topn(len(feats))
    flagged, pairs = g.last_stats()
    print("logbase %r, %s frames, %s: exact pass on %d of %d (frame, codebook-stream) pairs"
          % (base, batch, knobs, flagged, pairs))
    _same(got, ref)
    _same(gcw.astype(np.int32), rcw)


def test_ptm_is_refused_at_logbase_1_000015(models, means_en, means_fr):
    """T = 45, and with the weight bytes of en-us (158 at most) or of a mixture_weights file (159)
    the folded height is 164 and 255 + 96 + 3 x 45 = 486 < 512: the senone kernel's table would fit.
    But the reference's add table has 317 entries there, 256 to 316 all 1, and its log-add reads
    them (tests/test_settings_host.py shows chains that do); the kernels hold 256 and take 0
    beyond.  So the base is refused by name, before anything runs"""
    for model, means in (("en-us", means_en), ("fr-mixw", means_fr)):
        g, _ = models(model, {"logbase": 1.000015})
        wmax = int(g.table("ptm_mixw").max())
        tab = g.table("logadd8").astype(np.int64)
        assert wmax <= 159 and int((np.arange(wmax + 1) + tab[:wmax + 1]).max()) <= 255
        feats, off = _batch(means, BATCHES["130"], 6100)
        with pytest.raises(ssw.SswError, match=r"PTM scorer: unsupported log-add table \(317 entries"):
            g.score_batch(feats, off)


@pytest.fixture(scope="module")
def extreme_models(oracle_mod, orc_en, tmp_path_factory):
    """get(base) -> en-us under the 8-bit sendump of tests/test_gpu_senone_fold.py (weights 0 and
    255 side by side): wmax = 255, the folded table at its full height"""
    sd = str(tmp_path_factory.mktemp("settings_fold") / "sendump8")
    S.write_sendump8(sd, _extreme_weights(orc_en.n_feat, orc_en.n_density, orc_en.n_sen))
    kw = dict(mdef=os.path.join(SC.EN_US, "mdef"), means=os.path.join(SC.EN_US, "means"),
              sendump=sd, tmat=os.path.join(SC.EN_US, "transition_matrices"))
    var = os.path.join(SC.EN_US, "variances")
    cache = {}

    def get(base):
        if base not in cache:
            cache[base] = (ssw.Model(variances=var, config={"logbase": base}, **kw),
                           oracle_mod.Model(vars=var, config={"logbase": base}, **kw))
        return cache[base]
    yield get
    for g, _ in cache.values():
        g.close()


@pytest.mark.parametrize("knobs", ["default", "generic"])
@pytest.mark.parametrize("weights", ["en-us", "0-and-255"])
@pytest.mark.parametrize("base", [1.000018, 1.003])
def test_ptm_ties_and_far_frames_under_logbase(models, extreme_models, means_en, monkeypatch, base,
                                               weights, knobs):
    """the fold test's frames: half-way between two densities of a codebook (equal normalised
    scores), far from every density (features x 8: relative scores at the clamp) and ordinary
    ones; with en-us's weights and with weights 0 and 255 side by side, where at 1.000018 the
    folded height is 255 exactly"""
    _set(monkeypatch, KNOBS[knobs])
    g, o = models("en-us", {"logbase": base}) if weights == "en-us" else extreme_models(base)
    if weights != "en-us":
        tab = g.table("logadd8").astype(np.int64)
        assert int(g.table("ptm_mixw").max()) == 255 and int((np.arange(256) + tab).max()) == 255
    feats = _extreme_features(means_en)
    off = np.array([0, 40, 41, len(feats)], np.int32)
    ref, rcw, _ = _once(("ties", base, weights), lambda: _oracle_batch(o, feats, off))
    got = g.score_batch(feats, off)
    gcw, _ = g.last_topn(len(feats))
    _same(got, ref)
    _same(gcw.astype(np.int32), rcw)


# ---------------------------------------------------------------------------------------------
# the reference's recording under every recorded setting (logbase, varfloor, mixwfloor)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(SC.SCORING))
def test_recorded_rows(models, fx, case):
    """the reference's own rows: every frame's CRC, four frames whole; and the oracle's.  The
    mixwfloor cases are fr-fr's PTM weights quantised from the mixture_weights floats"""
    model, over = SC.SCORING[case]
    rec = fx["scoring"][case]
    g, o = models(model, over)
    feats = SC.features(model)
    assert rec["scorer"] == "ptm" and g.pick_scorer() == ssw.SCORER_PTM
    got = g.score_batch(feats)
    crcs = SC.row_crcs(got)
    bad = [t for t in range(len(got)) if crcs[t] != rec["row_crc"][t]]
    assert not bad, bad[:8]
    for t, want in rec["rows"].items():
        assert np.array_equal(got[int(t)], np.array(want, np.int16)), t
    ref, rcw, _ = _oracle_batch(o, feats, [0, len(feats)])
    gcw, _ = g.last_topn(len(feats))
    _same(got, ref)
    _same(gcw.astype(np.int32), rcw)


@pytest.mark.parametrize("batch", list(BATCHES))
@pytest.mark.parametrize("vf", [1e-2, 1.0])
def test_ptm_under_varfloor_both_instances(models, means_en, vf, batch):
    """both instances of the senone kernel; the first utterance's first 48 frames lie near the
    densities whose variances the floor raises (tests/test_settings_host.py: there the rows are
    not the default's)"""
    g, o = models("en-us", {"varfloor": vf})
    feats, off = _batch(means_en, BATCHES[batch], 6100)
    feats = feats.copy()
    feats[:48] = SC.floored_density_features(vf, 48, 31)
    ref, rcw, _ = _oracle_batch(o, feats, off)
    _same(g.score_batch(feats, off), ref)
    _same(g.last_topn(len(feats))[0].astype(np.int32), rcw)


# ---------------------------------------------------------------------------------------------
# the ms scorer (fr-fr with synthesised weights)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base,packed", [(1.00003, False), (1.00005, True), (1.003, True)])
def test_ms_under_logbase(models, means_fr, monkeypatch, base, packed):
    """2,049 frames: ms_senone_kernel at 1.00003 (255 + 640 + 6 x 23 = 1033 does not fit the
    mirrored table), the packed kernel at 1.00005 (979) and 1.003 (895).  The library has no
    interface that names the kernel a call ran, so the choice is pinned as far as bytes can pin
    it: the condition of ms_takes_packed_kernel recomputed from the model's own table, and the
    call's rows equal to those of a call that is made to take ms_senone_kernel
    (SSW_MS_SENONE=old) -- two kernels agreeing where two are expected, one run twice where one
    is: at 1.00003 the comparison is of ms_senone_kernel with itself, and what that case proves is
    the recomputed host condition and the rows, not which kernel ran.  The picked frames equal the
    oracle's.  Then 110 frames, the small-batch path."""
    g, o = models("fr-mixw", {"logbase": base})
    t_max = int(g.table("logadd8").max())
    assert (255 + 640 + 6 * t_max < 1024) == packed
    feats, off = _batch(means_fr, (1024, 1, 1024), 6400)
    ref = _once(("ms", base), lambda: o.ms_score_utt(feats[MS_PICK]))
    got = g.score_batch(feats, off, scorer=ssw.SCORER_MS)
    monkeypatch.setenv("SSW_MS_SENONE", "old")
    old = g.score_batch(feats, off, scorer=ssw.SCORER_MS)
    monkeypatch.delenv("SSW_MS_SENONE")
    assert (got.min(axis=1) == 0).all()
    _same(got, old)
    _same(got[MS_PICK], ref)
    small = g.score_batch(feats[:110], scorer=ssw.SCORER_MS)
    _same(small[:96], ref[:96])
    _same(small, got[:110])


@pytest.mark.parametrize("mf", [1e-3, 0.05])
def test_ms_under_mixwfloor(models, means_fr, mf):
    g, o = models("fr-mixw", {"mixwfloor": mf})
    feats = np.concatenate([SC.features("fr-mixw")[:48], synth_features(means_fr, 48, 77)])
    _same(g.score_batch(feats, [0, 48, 96], scorer=ssw.SCORER_MS), o.ms_score_utt(feats))


# ---------------------------------------------------------------------------------------------
# s2_semi (model A) and continuous (C3): numpy restatements over the library's tables
# ---------------------------------------------------------------------------------------------
def _file_tables(d):
    """(n_cb, veclen, n_density, means, variances) of a model directory, flat in file order"""
    n_cb, vl, ms = S.read_gauss(os.path.join(d, "means"))
    _, _, vs = S.read_gauss(os.path.join(d, "variances"))
    flat = lambda st: np.concatenate([s.reshape(n_cb, -1) for s in st], axis=1).reshape(-1)
    return n_cb, vl, ms[0].shape[1], flat(ms), flat(vs)


def _check_precompute(m, d, base):
    """mean, the scaled variances and det against gauden_dist_precompute restated in float32 /
    float64 as the reference types it (tests/mllr_common.restate), at this base"""
    n_cb, vl, nd, mean0, var0 = _file_tables(d)
    mean, var, det = M.restate(mean0, var0, vl, n_cb, nd, None, None, None, logbase=base)
    assert np.array_equal(m.table("mean"), mean)
    assert np.array_equal(m.table("var"), var)
    assert np.array_equal(m.table("det"), det)


@pytest.fixture(scope="module")
def other_dirs(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("settings_other"))
    return {"A": S.model_a_dir(os.path.join(tmp, "A")), "C3": CC.model_c3_dir(os.path.join(tmp, "C3"))}


@pytest.mark.parametrize("base", [1.00003, 1.003])
def test_s2_semi_under_logbase(other_dirs, oracle_mod, base):
    g = ssw.Model(other_dirs["A"], config={"logbase": base})
    try:
        assert g.scorer() == ssw.SCORER_S2_SEMI
        _check_precompute(g, other_dirs["A"], base)
        assert g.table("logadd8").tolist() == oracle_mod.Logmath(base, 10).table()[:256].tolist()
        feats = SC.features("en-us")[:64]
        r = S.restated_from_model(g)
        want = np.concatenate([r.utterance(feats[:41]), r.utterance(feats[41:])])
        _same(g.score_batch(feats, [0, 41, 64]), want)
    finally:
        g.close()


@pytest.mark.parametrize("base", [1.00003, 1.003])
def test_continuous_under_logbase(other_dirs, oracle_mod, base):
    g = ssw.Model(config={"logbase": base}, **CC.model_paths(other_dirs["C3"]))
    try:
        assert g.continuous
        _check_precompute(g, other_dirs["C3"], base)
        assert g.table("logadd8").tolist() == oracle_mod.Logmath(base, 10).table()[:256].tolist()
        feats = SC.features("en-us")[np.r_[0:24, 270:278]]
        want = CC.score_in_pieces(CC.restated_from_model(g), feats)
        _same(g.score_batch(feats, [0, 24, 32]), want)
    finally:
        g.close()


# ---------------------------------------------------------------------------------------------
# flows
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lexicons(models):
    cache = {}

    def get(over):
        key = tuple(sorted(over.items()))
        if key not in cache:
            cache[key] = ssw.Lexicon(models("en-us", over)[0], os.path.join(SC.EN_US, "dict.txt"),
                                     os.path.join(SC.EN_US, "noisedict.txt"))
        return cache[key]
    yield get
    for lex in cache.values():
        lex.free()


@pytest.mark.parametrize("case", [c for c, (kind, _, _) in SC.FLOWS.items() if kind == "align"])
def test_align_text_batch_under_the_setting(models, lexicons, oracle_mod, fx, case):
    """ssw_align_text_batch on the reference's recording: the words are the oracle's first pass
    over the oracle's rows, the states its second pass over the rows of the second scoring (the
    history carried over the rewind, as the reference's decoder carries it), and the JSON is the
    line the reference's decoder printed under the same setting"""
    _, _, over = SC.FLOWS[case]
    g, o = models("en-us", over)
    lex = lexicons(over)
    f39 = SC.features("en-us")
    n = len(f39)
    rows1 = o.ptm_score_utt(f39)
    rows2 = o.ptm_score_chain(f39, [0, n], reset=False)
    F, olex = _olex(oracle_mod, o, "en-us")
    want_seg = F.first_pass(o, olex, SC.TEXT, rows1)
    assert want_seg is not None
    want_words, want_st = _second_pass(g, lex, rows1, rows2, n)
    assert want_words == [w for (w, _, _, _) in want_seg]
    d_feats = torch.from_numpy(f39).cuda()
    aset = ssw.align_text_batch(g, lex, d_feats, [0, n], [SC.TEXT],
                                cfg=lex.first_pass_config(two_pass_history=1))
    try:
        assert aset.status(0) == 0, aset.message(0)
        got = aset.utterance(0)
        assert [(w, int(e[0]), int(e[0]) + int(e[1]) - 1) for w, e in zip(got["words"], got["word_al"])] \
            == [(w, s, e) for (w, s, e, _) in want_seg]
        assert np.array_equal(got["state_al"], want_st)
        assert aset.json(0, align_level=1).rstrip("\n") == fx["flows"][case]["json"].rstrip("\n")
    finally:
        aset.free()


def test_recognize_batch_at_logbase_1_0003(models, lexicons, oracle_mod, fx):
    """ssw_recognize_batch against tests/golden/fsg/goforward.fsg and against the text's chain
    grammar: the reference's hypothesis, score, segments and JSON of both, the grammar search
    over the oracle's rows, and the oracle's first pass"""
    over = {"logbase": 1.0003}
    g, o = models("en-us", over)
    lex = lexicons(over)
    f39 = SC.features("en-us")
    off = np.array([0, len(f39)], np.int32)
    rows = o.ptm_score_utt(f39)
    d_feats = torch.from_numpy(f39).cuda()
    d_rows = torch.from_numpy(rows).cuda()

    def against(rec, fsg):
        plan = lex.grammar_plan(fsg)
        r = ssw.recognize_batch(g, lex, d_feats, off, plan)
        want = ssw.grammar_search_batch(g, lex, d_rows, off, plan)
        assert r.status(0) == 0, r.message(0)
        assert _record(r, 0) == _record(want, 0)
        assert {"hyp": r.hyp(0), "score": r.score(0), "segments": [list(s) for s in r.segments(0)],
                "json": r.json(0)} \
            == {"hyp": rec["hyp"], "score": rec["score"], "segments": [s[:5] for s in rec["segments"]],
                "json": rec["json"]}
        return r

    against(fx["flows"]["rec_logbase_1.0003"], ssw.Fsg.read(g, lex, SC.FSG))
    chain = ssw.Fsg.create(g, lex, "chain", 0, len(SC.TEXT),
                           [(i, i + 1, 1.0, w) for i, w in enumerate(SC.TEXT)])
    rc = against(fx["flows"]["rec_chain_logbase_1.0003"], chain)
    F, olex = _olex(oracle_mod, o, "en-us")
    seg = F.first_pass(o, olex, SC.TEXT, rows)
    got, total = [], 0
    for w, sf, ef, ascr, lscr in rc.segments(0):
        total += ascr + lscr
        got.append((w, sf, ef, total))
    assert got == seg and rc.score(0) == seg[-1][3]


# ---------------------------------------------------------------------------------------------
# what is refused at the first scoring call
# ---------------------------------------------------------------------------------------------
def test_scoring_is_refused_by_name(models, extreme_models, other_dirs, means_en, means_fr):
    """the loader accepts 1.00001 and 1.000015 (the table's entries are bytes), but the reference's
    table has 515 and 317 entries there and its log-add reads all of them, where the kernels hold
    256: every scorer that adds with the table says so by name -- PTM (whatever the weights: with
    bytes up to 255 the folded height would not fit either), ms, s2_semi and the continuous
    models' ms -- and nothing is scored"""
    x_en, x_fr = synth_features(means_en, 8, 1), synth_features(means_fr, 8, 1)
    for base, entries in ((1.00001, 515), (1.000015, 317)):
        ptm = r"PTM scorer: unsupported log-add table \(%d entries, the kernels hold 256\)" % entries
        for g in (models("en-us", {"logbase": base})[0], extreme_models(base)[0]):
            with pytest.raises(ssw.SswError, match=ptm):
                g.score_batch(x_en)
        gf, _ = models("fr-mixw", {"logbase": base})
        with pytest.raises(ssw.SswError, match=ptm):
            gf.score_batch(x_fr)
        with pytest.raises(ssw.SswError, match=r"ms scorer: unsupported log base \(add table of %d "
                                                 r"entries\)" % entries):
            gf.score_batch(x_fr, scorer=ssw.SCORER_MS)
        ga = ssw.Model(other_dirs["A"], config={"logbase": base})
        gc = ssw.Model(config={"logbase": base}, **CC.model_paths(other_dirs["C3"]))
        try:
            with pytest.raises(ssw.SswError, match=r"s2_semi scorer: unsupported log-add table "
                                                     r"\(%d entries" % entries):
                ga.score_batch(x_en)
            with pytest.raises(ssw.SswError, match=r"unsupported log base \(add table of %d entries\)"
                                                     % entries):
                gc.score_batch(x_en)
        finally:
            ga.close()
            gc.close()
