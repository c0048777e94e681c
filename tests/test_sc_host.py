"""The loader and single-codebook (semi-continuous) models, host tables only (device =
SSW_DEVICE_NONE): they load, ssw_model_scorer names the s2_semi scorer, the derived tables are the
reference's, what is beyond the kernels' limits is refused by name -- and every model that loaded
before loads as before."""
import os
import zlib

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import sc_common as S
from tests.conftest import MODEL_ROOT

NONE = {"device": ssw.SSW_DEVICE_NONE}
# CRC-32 of en-us's host tables as the loader built them before single-codebook models loaded
EN_US_TABLES = {"rec": 3871578070, "scan_rec": 4134614820, "scan_rec_mfma": 3974842595,
                "scan_wfrag": 3803438924, "ptm_mixw": 536396333, "det": 2911970480,
                "scan_exact": 3800432154}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("sc_host"))
    d = {"A": S.model_a_dir(os.path.join(tmp, "A")), "B": S.model_b_dir(os.path.join(tmp, "B")),
         "A-ties": S.model_a_ties_dir(os.path.join(tmp, "A-ties"))}
    d["refused"] = S.refused_models(tmp)
    return d


def _crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def test_models_a_and_b_load_as_s2_semi(dirs):
    a = ssw.Model(dirs["A"], config=NONE)
    assert (a.n_cb, a.n_feat, a.n_density, a.veclen, a.n_sen) == (1, 3, 128, [13, 13, 13], 5126)
    assert a.scorer() == ssw.SCORER_S2_SEMI == 2 and a.has_ptm == 1
    b = ssw.Model(dirs["B"], config=NONE)
    assert (b.n_cb, b.n_feat, b.n_density, b.veclen) == (1, 4, 256, list(S.B_VECLEN))
    assert b.scorer() == ssw.SCORER_S2_SEMI
    # none of the PTM scan's tables
    for name in ("rec", "scan_rec", "scan_exact", "scan_rec_mfma", "scan_wfrag"):
        assert a.table(name).size == 0 and b.table(name).size == 0, name
    # the mixture weights are the sendump's bytes
    assert np.array_equal(b.table("ptm_mixw").reshape(4, 256, 5126), S.model_b_tables()[2])
    assert np.array_equal(a.table("ptm_mixw"),
                          S.read_sendump8(os.path.join(S.EN_US, "sendump")).ravel())


def test_model_path_and_scorer_of_the_shipped_models():
    for name in ("en-us", "fr-fr"):
        m = ssw.Model(os.path.join(MODEL_ROOT, name), config=NONE)
        assert m.scorer() == ssw.SCORER_PTM
    assert _lib.lib().ssw_abi_version() == 2


def test_en_us_tables_hash_as_before():
    m = ssw.Model(os.path.join(MODEL_ROOT, "en-us"), config=NONE)
    assert {k: _crc(m.table(k)) for k in EN_US_TABLES} == EN_US_TABLES


@pytest.mark.parametrize("case", ["A", "A-ties", "B"])
def test_det_and_variances_are_the_references(dirs, case):
    """CRC-32 of det and of the scaled variances as the reference's gauden_t holds them: a libm
    that differs in a last place shows here, not in a kernel test"""
    fx = S.results()["scoring"][case]
    m = ssw.Model(dirs[case], config=NONE)
    assert _crc(m.table("det")) == fx["det_crc"]
    assert _crc(m.table("var")) == fx["var_crc"]


@pytest.mark.parametrize("name", ["topn5", "257_densities", "33_dimensions",
                                  "20_dimensions_42_codebooks"])
def test_refused_by_name(dirs, name):
    d, topn, words = dirs["refused"][name]
    with pytest.raises(ssw.SswError) as e:
        ssw.Model(d, config=dict(NONE, topn=topn))
    for w in words:
        assert w in str(e.value), str(e.value)


def test_topn_1_to_4_and_any_ds_load(dirs):
    for topn in (1, 2, 3, 4):
        m = ssw.Model(dirs["A"], config=dict(NONE, topn=topn, ds=3))
        assert m.topn == topn and m.scorer() == ssw.SCORER_S2_SEMI


def test_clustered_sendump_expands_by_senone_parity(dirs, tmp_path):
    """the s2_semi scorer takes senone j's 4-bit code from the low nibble of byte j / 2 for an even
    j and from the high nibble for an odd one (get_scores_4b_feat_all); ptm_mgau keys the choice
    on the byte's own low bit.  A single-codebook model expands the first way."""
    d = S.model_a_dir(str(tmp_path / "A4"))
    u = S.lcg_uniform(99, 3 * 128 * 5126)
    codes = np.floor(u * 16).astype(np.uint8).reshape(3, 128, 5126)
    codebook = np.array([0, 3, 7, 12, 18, 25, 33, 42, 52, 63, 75, 88, 102, 117, 133, 150], np.uint8)
    S.write_sendump4(os.path.join(d, "sendump"), codebook, codes)
    m = ssw.Model(d, config=NONE)
    assert m.scorer() == ssw.SCORER_S2_SEMI
    assert np.array_equal(m.table("ptm_mixw").reshape(3, 128, 5126), codebook[codes])
