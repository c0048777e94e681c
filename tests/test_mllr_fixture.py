"""The MLLR fixture recorded from the reference (tests/golden/make_mllr.py) against the numpy
restatement of the transform (tests/mllr_common.restate) and, for the continuous models, against
cont_common.Restated over the adapted tables: the fixture and the arithmetic agree before a GPU
is involved."""
import numpy as np
import pytest

import soundswallower_amd as ssw
from tests import cont_common as CC
from tests import mllr_common as M
from tests.test_mllr_host import S_read, read

NONE = ssw.SSW_DEVICE_NONE


@pytest.fixture(scope="module")
def kwargs(tmp_path_factory):
    from soundswallower_amd import _lib
    _lib.build()
    return M.model_kwargs(str(tmp_path_factory.mktemp("mllr_models")))


@pytest.fixture(scope="module")
def fx():
    return M.results()


def test_fixture_is_complete(fx):
    assert fx["scale"] == 1.0
    for model, (_, scorer) in M.MODELS.items():
        for name in M.TRANSFORMS:
            rec = fx["scoring"]["%s/%s" % (model, name)]
            assert rec["scorer"] == scorer and rec["frames"] == 278 and len(rec["row_crc"]) == 278
            assert sorted(rec["rows"], key=int) == ["0", "1", "2", "277"]
        sc = fx["scoring"]
        assert sc[model + "/two_class"]["row_crc"] == sc[model + "/mild"]["row_crc"]
        for other in ("mild", "var", "floor"):
            assert sc[model + "/" + other]["row_crc"] != sc[model + "/identity"]["row_crc"]
    for model in ("en-us", "C3"):
        for name in ("mild", "var"):
            assert '"w":[' in fx["align"]["%s/%s" % (model, name)]["json"]
            for g in M.GRAMMARS:
                assert fx["rec"]["%s/%s/%s" % (model, name, g)]["hyp"]
    assert all(fx["rec_default"][g]["hyp"] for g in M.GRAMMARS) and fx["align_default"]["json"]


def test_restated_tables_have_the_recorded_crcs(kwargs, fx):
    for model, (layout, _) in M.MODELS.items():
        m = M.load(kwargs[model], NONE)
        mean0, var0 = S_read(kwargs[model])
        for name in M.TRANSFORMS:
            rec = fx["scoring"]["%s/%s" % (model, name)]
            _, var, det = M.restate(mean0, var0, m.veclen, m.n_cb, m.n_density,
                                    *read(name, layout).arrays(0))
            assert (M.crc(det), M.crc(var)) == (rec["det_crc"], rec["var_crc"]), (model, name)
        m.close()


@pytest.mark.parametrize("model", ["C3", "C1"])
def test_continuous_rows_from_the_adapted_tables(kwargs, fx, model):
    layout = M.MODELS[model][0]
    m = M.load(kwargs[model], NONE)
    feats = M.features(model)
    pick = [0, 1, 2, 277]
    for name in ("mild", "var", "floor"):
        rec = fx["scoring"]["%s/%s" % (model, name)]
        m.apply_mllr(read(name, layout))
        r = CC.restated_from_model(m)
        if name == "mild":  # every frame once; the other transforms on the frames recorded whole
            assert CC.row_crcs(CC.score_in_pieces(r, feats)) == rec["row_crc"], (model, name)
        got = r.score(feats[pick])
        for t, row in zip(pick, got):
            assert row.tolist() == rec["rows"][str(t)], (model, name, t)
    m.close()
