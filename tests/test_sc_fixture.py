"""The fixtures of the s2_semi (single-codebook) tests: the committed cut of en-us (model A), the
reference's recorded scoring, recognition and alignment (tests/golden/sc_results.json, written by
tests/golden/make_sc.py), and the plain numpy restatement of the scorer (tests/sc_common.py)
against every recorded row.  A mismatch in the last group is a wrong restatement: the GPU tests
compare the kernels with it wherever the reference recorded nothing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import sc_common as S
from tests.conftest import ROOT

GENERATOR = os.path.join(S.GOLD, "make_sc.py")
CASES = ["A", "A-ties", "B"] + ["A_topn%d_ds%d" % s for s in S.SETTINGS]


@pytest.fixture(scope="module")
def models(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("sc_models"))
    return {"A": S.model_a_dir(os.path.join(tmp, "A")),
            "A-ties": S.model_a_ties_dir(os.path.join(tmp, "A-ties")),
            "B": S.model_b_dir(os.path.join(tmp, "B"))}


def test_model_a_is_the_cut_of_our_en_us_files(tmp_path):
    for n in ("means", "variances"):
        p = str(tmp_path / n)
        S.cut_codebook(os.path.join(S.EN_US, n), p)
        with open(p, "rb") as a, open(os.path.join(S.MODEL_A, n), "rb") as b:
            blob = a.read()
            assert blob == b.read(), n
        assert len(blob) == 20038
        n_cb, vl, streams = S.read_gauss(p)
        assert (n_cb, vl, streams[0].shape) == (1, (13, 13, 13), (1, 128, 13))
    with open(os.path.join(S.EN_US, "feat_params.json"), "rb") as a, \
            open(os.path.join(S.MODEL_A, "feat_params.json"), "rb") as b:
        assert a.read() == b.read()


def test_the_fixture_has_exactly_the_cases():
    fx = S.results()
    assert sorted(fx["scoring"]) == sorted(CASES)
    for name, rec in fx["scoring"].items():
        assert rec["scorer"] == "s2_semi", name
        frames = S.B_FRAMES if name == "B" else 278
        assert rec["frames"] == frames and len(rec["row_crc"]) == frames, name
        assert sorted(rec["rows"], key=int) == ["0", "1", "2", str(frames - 1)], name
        assert all(len(r) == 5126 for r in rec["rows"].values()), name
    assert sorted(fx["rec"]) == ["goforward", "loop", "nulls"] and sorted(fx["align"]) == ["no", "yes"]
    assert os.path.getsize(S.RESULTS_JSON) < (1 << 20)
    assert np.load(S.FEAT_A).shape == (278, 39) and np.load(S.FEAT_A).dtype == np.float32


def test_the_two_configurations_are_the_same_computation():
    """s2_semi_mgau_frame_eval evaluates every Gaussian and normalises per stream whatever the
    active set is: compallsen = no and yes recognise and align identically"""
    fx = S.results()
    want = {"goforward": ("go forward ten meters", -32145), "loop": ("a go a a ten meters", -32214),
            "nulls": ("go forward ten meters", -32320)}
    for g, (hyp, score) in want.items():
        assert fx["rec"][g]["yes"] == fx["rec"][g]["no"], g
        assert (fx["rec"][g]["yes"]["hyp"], fx["rec"][g]["yes"]["score"]) == (hyp, score), g
        assert fx["rec"][g]["yes"]["scorer"] == "s2_semi"
    assert fx["align"]["yes"] == fx["align"]["no"]
    assert fx["align"]["yes"]["json"].startswith(
        '{"b":0.000,"d":2.790,"p":1.000,"t":"go forward ten meters","w":[{"b":0.000,"d":0.450,'
        '"p":0.626,"t":"<sil>"')


def test_generator_check_mode_agrees_with_the_reference_build():
    from oracle import reference
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, GENERATOR, "--check"], cwd=ROOT, capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_the_recorded_features_are_the_front_end_of_the_mfcc_fixture(oracle_mod):
    """the 278 rows the reference scored = 1s_c_d_dd with batch CMN over goforward_mfcc.npy (what
    ssw_feat_batch computes on the GPU)"""
    cep = np.load(os.path.join(S.GOLD, "goforward_mfcc.npy")).astype(np.float32)
    assert np.array_equal(oracle_mod.feat_1s_c_d_dd(cep), np.load(S.FEAT_A))


@pytest.mark.parametrize("case", CASES)
def test_the_restatement_reproduces_every_recorded_row(models, case):
    fx = S.results()["scoring"][case]
    if case == "B":
        topn, ds, d = 4, 1, models["B"]
        feats = S.model_b_features(S.model_b_tables()[0])
    else:
        topn, ds = (4, 1) if "_" not in case else (int(case[6]), int(case[-1]))
        d, feats = models["A-ties" if case == "A-ties" else "A"], np.load(S.FEAT_A)
    m = ssw.Model(d, config={"device": ssw.SSW_DEVICE_NONE, "topn": topn, "ds": ds})
    rows = S.restated_from_model(m, topn, ds).utterance(feats)
    got = S.row_crcs(rows)
    bad = [t for t in range(len(got)) if got[t] != fx["row_crc"][t]]
    assert not bad, "frames %s ... differ from the reference's" % bad[:8]
    for t, row in fx["rows"].items():
        assert np.array_equal(rows[int(t)], np.array(row, np.int16)), t


def test_the_ties_model_is_where_the_accept_rule_decides(models):
    """with PTM's accept rule (d >= worst as floats: a density whose score truncates to the worst
    entry's is rejected unless it is an integer) the restatement leaves the recorded rows of model
    A-ties: the fixture tells the two rules apart"""
    fx = S.results()["scoring"]["A-ties"]
    m = ssw.Model(models["A-ties"], config={"device": ssw.SSW_DEVICE_NONE})
    r = S.restated_from_model(m)
    r.ptm_rule = True
    got = S.row_crcs(r.utterance(np.load(S.FEAT_A)))
    assert got != fx["row_crc"]
