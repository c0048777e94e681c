"""The loader and continuous-density models (one codebook per senone), host tables only (device =
SSW_DEVICE_NONE): they load as continuous and as the ms scorer's, the derived tables are the
reference's, sen2cb is the identity, every limit is refused by name -- and the shipped models load
as before."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import cont_common as CC
from tests.conftest import MODEL_ROOT

NONE = {"device": ssw.SSW_DEVICE_NONE}


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("cont_host"))
    d = {n: b(os.path.join(tmp, n)) for n, b in CC.BUILDERS.items()}
    d["tmp"] = tmp
    return d


def _load(d, mdef=True, sendump=None, **cfg):
    return ssw.Model(**CC.model_paths(d, mdef), sendump=sendump, config=dict(NONE, **cfg))


def test_c3_and_c1_load_as_continuous_ms(dirs):
    c3 = _load(dirs["C3"])
    assert (c3.n_cb, c3.n_feat, c3.n_density, c3.veclen, c3.n_sen) == (5126, 3, 8, [13, 13, 13], 5126)
    c1 = _load(dirs["C1"])
    assert (c1.n_cb, c1.n_feat, c1.n_density, c1.veclen, c1.n_sen) == (5126, 1, 6, [39], 5126)
    for m in (c3, c1):
        assert m.continuous and m.scorer() == ssw.SCORER_MS == 1 and m.pick_scorer() == ssw.SCORER_MS
        assert m.has_ms == 1 and m.has_ptm == 0
        assert np.array_equal(m.table("sen2cb"), np.arange(5126, dtype=np.int16))
        # none of the PTM scan's tables
        for name in ("rec", "scan_rec", "scan_exact", "scan_rec_mfma", "scan_wfrag", "ptm_mixw"):
            assert m.table(name).size == 0, name
    assert _lib.lib().ssw_abi_version() == 2


def test_topn_outside_the_densities_means_all(dirs):
    assert _load(dirs["C1"], topn=0).topn == 6 and _load(dirs["C1"], topn=7).topn == 6
    assert _load(dirs["C3"], topn=3).topn == 3


@pytest.mark.parametrize("case", ["C3", "C3-ties", "C1", "C3_mixwfloor"])
def test_det_and_variances_are_the_references(dirs, case):
    """CRC-32 of det and of the scaled variances as the reference's gauden_t holds them: a libm
    that differs in a last place shows here, not in a kernel test"""
    fx = CC.results()["scoring"][case]
    m = _load(dirs[CC.CASES[case][0]])
    assert CC.crc(m.table("det")) == fx["det_crc"]
    assert CC.crc(m.table("var")) == fx["var_crc"]


def test_ms_pdf_is_the_weights_quantised_as_senone_mixw_read_does(dirs):
    """pdf = (-(int) logs3(w) + 511) >> 10, 255 at most, of the weights normalised, floored and
    normalised again (src/ms_senone.c:156-182); C3's weights are logbase^-(q << 10) of the eight
    smallest q, so the quantised values are q shifted by the normaliser"""
    m = _load(dirs["C3"])
    pdf = m.table("ms_pdf").reshape(5126, 3, 8).astype(np.int64)
    _, _, w = CC.c3_tables()
    w = w.astype(np.float64)
    w = w / w.sum(axis=2, keepdims=True)
    want = np.minimum((-np.log(w) / np.log(CC.LOGBASE)).astype(np.int64) + 511 >> 10, 255)
    # (float32 renormalisation in the loader: a weight on a rounding boundary may move by one)
    assert np.abs(pdf - want).max() <= 1 and np.count_nonzero(pdf != want) < pdf.size // 1000


def _refused(words, **kw):
    with pytest.raises(ssw.SswError) as e:
        _load(**kw)
    for w in words:
        assert w in str(e.value), str(e.value)


def test_limits_are_refused_by_name(dirs):
    tmp = dirs["tmp"]
    syn = lambda name, *a, **k: CC.synthetic_dir(os.path.join(tmp, name), *a, **k)
    _refused(("continuous", "65 dimensions"), d=syn("v65", 4, (3, 65), 2, 1), mdef=False)
    _refused(("continuous", "65 densities"), d=syn("d65", 4, (3,), 65, 2), mdef=False)
    _refused(("continuous", "topn 9"), d=syn("t9", 4, (3,), 12, 3), mdef=False, topn=9)
    _refused(("5 codebooks for 4 senones", "more codebooks"), d=syn("cb5", 4, (3,), 2, 4, n_cb=5),
             mdef=False)
    _refused(("3 codebooks for 4 senones", "fewer codebooks"), d=syn("cb3", 4, (3,), 2, 5, n_cb=3),
             mdef=False)
    # the limits themselves load: 64 dimensions, 64 densities, topn 8 and topn = all
    assert _load(syn("v64", 4, (3, 64), 2, 6), mdef=False).continuous
    assert _load(syn("d64", 4, (3,), 64, 7), mdef=False, topn=8).continuous
    m = _load(syn("d12", 4, (3,), 12, 8), mdef=False, topn=12)
    assert m.continuous and m.topn == 12 and m.n_sen == 4


def test_nine_streams_are_refused(dirs):
    _refused(("9",), d=CC.synthetic_dir(os.path.join(dirs["tmp"], "f9"), 4, (2,) * 9, 2, 9),
             mdef=False)


def test_a_sendump_with_a_continuous_model_is_refused(dirs):
    _refused(("continuous", "sendump"), d=dirs["C3"],
             sendump=os.path.join(MODEL_ROOT, "en-us", "sendump"))


def test_shipped_models_are_not_continuous():
    for name in ("en-us", "fr-fr"):
        m = ssw.Model(os.path.join(MODEL_ROOT, name), config=NONE)
        assert not m.continuous and m.scorer() == ssw.SCORER_PTM


def test_scoring_without_a_device_is_refused(dirs):
    m = _load(dirs["C1"])
    with pytest.raises(ssw.SswError, match="SSW_DEVICE_NONE"):
        m.score_batch(np.zeros((2, 39), np.float32))
