"""MLLR speaker adaptation on the GPU: every scorer family under every fixture transform against
the rows the reference recorded (tests/golden/mllr_results.json, tests/golden/make_mllr.py), on
both top-N scans and the chain kernel for en-us; identity and apply(None) against the goldens of
the unadapted models; one model object through a sequence of transforms; alignment and
recognition under adaptation; the drop-in's transform slot; a refused transform."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import cont_common as CC
from tests import mllr_common as M
from tests import sc_common as S

pytestmark = pytest.mark.gpu

WORDS = ["go forward ten meters".split()]


@pytest.fixture(scope="module")
def kwargs(tmp_path_factory):
    _lib.build()
    return M.model_kwargs(str(tmp_path_factory.mktemp("mllr_gpu")))


@pytest.fixture(scope="module")
def fx():
    return M.results()


@pytest.fixture(scope="module")
def models(kwargs):
    """one device model per family, loaded when first asked for, shared by the tests: each test
    applies what it needs"""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = M.load(kwargs[name], -1)
        return cache[name]
    yield get
    for m in cache.values():
        m.close()


def read(name, model):
    return ssw.Mllr.read(M.transform_path(name, M.MODELS[model][0]))


def scorer_of(model):
    return ssw.SCORER_MS if model == "fr-fr" else None


_fr_rows = {}


def features(m, model):
    """the 278 feature rows of goforward.raw: the recorded ones of en-us's 39-dimensional front
    end; for fr-fr what the model's own front end makes of the recording, which has to be what
    the reference scored (tests/golden/mllr/goforward_fr_feat.npy)"""
    if model != "fr-fr":
        return M.features(model)
    if not _fr_rows:
        cep, _ = m.fe_batch(np.fromfile(M.PCM, dtype="<i2"))
        _fr_rows["x"] = np.ascontiguousarray(m.feat_batch(cep), np.float32)
        assert np.array_equal(_fr_rows["x"], M.features("fr-fr")), \
            "fr-fr's front end does not give the rows the reference scored"
    return _fr_rows["x"]


def rows(m, model):
    return m.score_batch(features(m, model), scorer=scorer_of(model))


def check_rows(got, rec, what=""):
    crcs = CC.row_crcs(got)
    bad = [t for t in range(len(crcs)) if crcs[t] != rec["row_crc"][t]]
    assert not bad, "%s: frames %s ... differ from the reference's" % (what, bad[:8])
    for t, row in rec["rows"].items():
        assert np.array_equal(got[int(t)], np.array(row, np.int16)), (what, t)


# ---- scoring -------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", sorted(M.MODELS))
@pytest.mark.parametrize("name", M.TRANSFORMS)
def test_recorded_rows(models, fx, model, name):
    m = models(model)
    gen = m.mllr_generation
    m.apply_mllr(read(name, model))
    assert m.mllr_generation == gen + 1
    check_rows(rows(m, model), fx["scoring"]["%s/%s" % (model, name)], model + "/" + name)


@pytest.mark.parametrize("name", ["mild", "var", "floor"])
def test_en_us_on_both_scans(models, fx, name, monkeypatch):
    m = models("en-us")
    m.apply_mllr(read(name, "en-us"))
    rec = fx["scoring"]["en-us/" + name]
    feats = M.features("en-us")
    assert m.scan_mode == 1, m.selftest_message  # the matrix-core scan is what a batch takes
    check_rows(m.score_batch(feats), rec, "matrix-core scan")
    # the recording three times over as three utterances of one batch
    tiled = np.concatenate([feats, feats, feats])
    got = m.score_batch(tiled, utt_off=[0, 278, 556, 834])
    for k in range(3):
        check_rows(got[278 * k:278 * (k + 1)], rec, "matrix-core scan, utterance %d" % k)
    monkeypatch.setenv("SSW_SCAN", "fma")
    check_rows(m.score_batch(feats), rec, "vector-unit scan")
    monkeypatch.delenv("SSW_SCAN")
    monkeypatch.setenv("SSW_MFMA_MIN_FRAMES", "100000")
    check_rows(m.score_batch(feats), rec, "below the matrix-core threshold")


def test_en_us_chain_kernel_ds2(kwargs, fx):
    """ds = 2 takes the sequential chain kernel; the transform comes through Model(mllr=)"""
    m = ssw.Model(S.EN_US, config={"ds": 2}, mllr=M.transform_path("mild", "3x13"))
    assert m.mllr_generation == 1
    check_rows(m.score_batch(M.features("en-us")), fx["scoring"]["en-us_ds2/mild"], "ds = 2")
    m.close()


def test_identity_and_clear_give_the_unadapted_goldens(models, fx):
    old = {"cb41": S.results()["scoring"]["A"], "C3": CC.results()["scoring"]["C3"],
           "C1": CC.results()["scoring"]["C1"]}
    for model in sorted(M.MODELS):
        m = models(model)
        # (the generator holds <model>/identity to the reference without a transform; the three
        # models with earlier fixtures are held to those as well)
        want = [fx["scoring"][model + "/identity"]] + ([old[model]] if model in old else [])
        m.apply_mllr(read("var", model))
        m.apply_mllr(read("identity", model))
        got = rows(m, model)
        for rec in want:
            check_rows(got, rec, model + " identity")
        m.apply_mllr(read("var", model))
        m.apply_mllr(None)
        got = rows(m, model)
        for rec in want:
            check_rows(got, rec, model + " cleared")


@pytest.mark.parametrize("model", sorted(M.MODELS))
def test_one_model_through_mild_var_mild(models, fx, model):
    """a table left behind by the previous upload would show in the next call's rows"""
    m = models(model)
    for name in ("mild", "var", "mild", "floor", "mild"):
        m.apply_mllr(read(name, model))
        check_rows(rows(m, model), fx["scoring"]["%s/%s" % (model, name)], model + "/" + name)


def test_refused_transform_leaves_the_scores(models, fx):
    m = models("en-us")
    m.apply_mllr(read("mild", "en-us"))
    gen = m.mllr_generation
    with pytest.raises(ssw.SswError, match="1 feature streams, the model has 3"):
        m.apply_mllr(ssw.Mllr.read(M.transform_path("var", "1x39")))
    eye = [np.eye(13, dtype=np.float32)] * 3
    with pytest.raises(ssw.SswError, match="stream 1 has 12 dimensions"):
        m.apply_mllr(ssw.Mllr(A=[eye[0], np.eye(12), eye[0]],
                              b=[np.zeros(13), np.zeros(12), np.zeros(13)],
                              h=[np.ones(13), np.ones(12), np.ones(13)]))
    assert m.mllr_generation == gen
    check_rows(rows(m, "en-us"), fx["scoring"]["en-us/mild"], "after a refusal")


# ---- alignment and recognition ---------------------------------------------------------------------
def lexicon(m, kwargs, model):
    d = S.EN_US if model == "en-us" else os.path.dirname(kwargs[model]["means"])
    return ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))


def recognise(m, lex, grammar, active=False):
    pcm = np.fromfile(M.PCM, dtype="<i2")
    plan = lex.grammar_plan(ssw.Fsg.read(m, lex, os.path.join(M.GOLD, "fsg", grammar + ".fsg")))
    r = ssw.recognize_audio_batch(m, lex, pcm, [0, len(pcm)], plan, active=active)
    assert r.status(0) == 0, r.message(0)
    got = {"hyp": r.hyp(0), "score": r.score(0), "segments": [list(s) for s in r.segments(0)],
           "json": r.json(0)}
    r.free()
    return got


def recorded(rec):
    return {"hyp": rec["hyp"], "score": rec["score"], "segments": [s[:5] for s in rec["segments"]],
            "json": rec["json"]}


def align(m, lex, active=False):
    pcm = np.fromfile(M.PCM, dtype="<i2")
    a = ssw.align_audio_batch(m, lex, pcm, [0, len(pcm)], WORDS, active=active)
    assert a.status(0) == 0, a.message(0)
    js = a.json(0).rstrip("\n")
    a.free()
    return js


@pytest.mark.parametrize("model", ["en-us", "C3"])
def test_align_and_recognize_under_adaptation(models, kwargs, fx, model):
    m = models(model)
    lex = lexicon(m, kwargs, model)
    for name in ("mild", "var"):
        m.apply_mllr(read(name, model))
        assert align(m, lex) == fx["align"]["%s/%s" % (model, name)]["json"].rstrip("\n"), name
        for g in M.GRAMMARS:
            assert recognise(m, lex, g) == recorded(fx["rec"]["%s/%s/%s" % (model, name, g)]), \
                (name, g)


def test_default_configuration_under_adaptation(models, kwargs, fx):
    m = models("en-us")
    lex = lexicon(m, kwargs, "en-us")
    m.apply_mllr(read("mild", "en-us"))
    assert align(m, lex, active=True) == fx["align_default"]["json"].rstrip("\n")
    for g in M.GRAMMARS:
        assert recognise(m, lex, g, active=True) == recorded(fx["rec_default"][g]), g


# ---- the drop-in ---------------------------------------------------------------------------------
@pytest.mark.parametrize("model,cls,vt", [("en-us", "PtmMgau", "ptm"), ("fr-fr", "MsMgau", "ms"),
                                          ("C3", "MsMgau", "ms"), ("cb41", "S2SemiMgau", "s2_semi")])
def test_drop_in_transform(models, fx, model, cls, vt):
    m = models(model)
    m.apply_mllr(None)
    feats = features(m, model)
    g = getattr(ssw, cls)(m)
    assert g.name == vt
    base = fx["scoring"][model + "/identity"]
    mild = fx["scoring"][model + "/mild"]

    def first_rows(n=3):
        g.reset_hist()
        out = []
        for t in range(n):
            g.frame_idx = t
            out.append(g.frame_eval(feats[t], t))
        return out

    for t, row in enumerate(first_rows()):
        assert row.tolist() == base["rows"][str(t)], t
    assert g.transform() == -1  # NULL, as before: the model does not move
    gen = m.mllr_generation
    g.prescore(feats)
    assert g.frame_eval(feats[277], 277).tolist() == base["rows"]["277"]
    assert g.transform(read("mild", model)) == 0 and m.mllr_generation == gen + 1
    # the rows prescore held are the old parameters': not served
    g.frame_idx = 277
    for t, row in enumerate(first_rows()):
        assert row.tolist() == mild["rows"][str(t)], t
    g.prescore(feats)
    check_rows(np.stack([g.frame_eval(feats[t], t) for t in range(len(feats))]), mild, model)
    # a transform that does not fit: -1, and the scorer keeps its rows
    other = ssw.Mllr.read(M.transform_path("mild", "1x39" if M.MODELS[model][0] == "3x13" else "3x13"))
    assert g.transform(other) == -1 and "feature streams" in _lib.last_error()
    assert m.mllr_generation == gen + 1
    assert g.frame_eval(feats[277], 277).tolist() == mild["rows"]["277"]
    # a transform applied to the model itself, not through the slot: the prescored rows are not
    # the model's any more and are not served either
    m.apply_mllr(None)
    g.frame_idx = 277
    for t, row in enumerate(first_rows()):
        assert row.tolist() == base["rows"][str(t)], t
    m.apply_mllr(read("mild", model))
    g.free()
    check_rows(rows(m, model), mild, model + " batch after the drop-in's transform")
