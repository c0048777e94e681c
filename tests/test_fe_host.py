"""The MFCC front end's host side (no GPU): the framing rule of ssw_fe_frame_count against the
oracle's restatement of fe_process_int16 + fe_end, the configuration ssw_model_load reads from
feat_params.json, and the arguments and configurations ssw_fe_batch refuses."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests.conftest import MODEL_ROOT


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cpu_en(lib):
    return ssw.Model(os.path.join(MODEL_ROOT, "en-us"), config={"device": -2})


def test_frame_count_matches_the_oracle(lib, cpu_en, oracle_mod):
    rng = np.random.default_rng(8)
    lengths = list(range(0, 2001)) + [int(x) for x in rng.integers(2001, 200000, 40)] + [44580]
    pcm = rng.integers(-3000, 3000, max(lengths)).astype(np.int16)
    for n in lengths:
        want = len(oracle_mod.fe_mfcc(pcm[:n]))
        assert lib.ssw_fe_frame_count(cpu_en._m, n) == want, n
        assert ssw.fe_frame_counts([n])[0] == want, n
    assert lib.ssw_fe_frame_count(cpu_en._m, 44580) == 278
    assert lib.ssw_fe_frame_count(cpu_en._m, -1) == -1
    assert lib.ssw_fe_frame_count(None, 100) == -1


@pytest.mark.parametrize("name", ["en-us", "fr-fr"])
def test_model_reads_feat_params_json(lib, name):
    m = ssw.Model(os.path.join(MODEL_ROOT, name), config={"device": -2})
    got = m.fe_config()
    want = json.load(open(os.path.join(MODEL_ROOT, name, "feat_params.json")))
    assert got.from_file == 1
    assert got.nfilt == want["nfilt"] and got.lifter == want["lifter"]
    assert got.lowerf == want["lowerf"] and got.upperf == want["upperf"]
    assert got.transform == ssw.api.FE_TRANSFORMS[want["transform"]]
    assert got.remove_noise == int(want["remove_noise"])
    # keys the front end does not set keep the reference's defaults
    assert (got.samprate, got.frate, got.ncep, got.nfft) == (16000, 100, 13, 0)
    assert abs(got.wlen - 0.025625) < 1e-12 and abs(got.alpha - 0.97) < 1e-12
    assert (got.dither, got.remove_dc, got.warp, got.unit_area, got.round_filters) == (0, 0, 0, 1, 1)


def _model_with_params(tmp_path, params):
    """the en-us model's files beside a feat_params.json of our own"""
    src = os.path.join(MODEL_ROOT, "en-us")
    for f in ("mdef", "means", "variances", "sendump", "transition_matrices"):
        os.symlink(os.path.join(src, f), tmp_path / f)
    if params is not None:
        (tmp_path / "feat_params.json").write_text(params)
    return ssw.Model(str(tmp_path), config={"device": -2})


def test_missing_feat_params_gives_the_reference_defaults(tmp_path):
    c = _model_with_params(tmp_path, None).fe_config()
    assert c.from_file == 0
    assert (c.nfilt, c.lifter, c.transform, c.remove_noise) == (40, 0, 0, 0)
    assert np.float32(c.lowerf) == np.float32(133.33334)
    assert np.float32(c.upperf) == np.float32(6855.4976)


def test_unused_and_refused_keys_do_not_fail_the_load(tmp_path):
    m = _model_with_params(tmp_path, json.dumps({
        "-nfilt": 25, "transform": "htk", "dither": "yes", "feat": "1s_c_d_dd", "cmn": "live",
        "agc": "none", "warp_params": "", "remove_dc": False, "samprate": "16000"}))
    c = m.fe_config()
    assert (c.from_file, c.nfilt, c.transform, c.dither, c.warp) == (1, 25, 2, 1, 0)
    with pytest.raises(ssw.SswError, match="htk"):
        m.fe_batch(np.zeros(1000, np.int16))


def test_unusable_feat_params_is_reported_by_the_front_end_only(tmp_path):
    m = _model_with_params(tmp_path, '{"nfilt": "many"}')
    assert m.n_sen > 0 and m.fe_config().from_file == 0
    with pytest.raises(ssw.SswError, match="feat_params.json"):
        m.fe_batch(np.zeros(1000, np.int16))
    # an explicit configuration does not need the file
    with pytest.raises(ssw.SswError, match="no GPU"):
        m.fe_batch(np.zeros(1000, np.int16), cfg={"nfilt": 20})


@pytest.mark.parametrize("over,msg", [
    ({"transform": "htk"}, "htk"), ({"dither": 1}, "dither"), ({"remove_dc": 1}, "remove_dc"),
    ({"smoothspec": 1}, "smoothspec"), ({"logspec": 1}, "logspec"), ({"warp": 1}, "warp"),
    ({"doublebw": 1}, "doublebw"), ({"samprate": 8000.0}, "samprate 16000"),
    ({"frate": 50}, "frate"), ({"wlen": 0.02}, "wlen"), ({"nfft": 1024}, "FFT"),
    ({"ncep": 12}, "ncep"), ({"alpha": 0.95}, "alpha"), ({"nfilt": 65}, "nfilt"),
    ({"nfilt": 0}, "nfilt"), ({"lifter": -1}, "lifter"), ({"upperf": 9000.0}, "upperf"),
    ({"lowerf": 4000.0, "upperf": 3000.0}, "lowerf"), ({"lowerf": -1.0}, "lowerf"),
    ({"unit_area": 0}, "unit_area"), ({"round_filters": 0}, "round_filters")])
def test_unsupported_configurations_are_refused(cpu_en, over, msg):
    with pytest.raises(ssw.SswError, match=msg):
        cpu_en.fe_batch(np.zeros(1000, np.int16), cfg=over)


def test_bad_arguments_are_refused(lib, cpu_en):
    fo = np.zeros(3, np.int32)
    for off in ([1, 5, 9], [0, 9, 5]):
        o = np.array(off, np.int64)
        assert lib.ssw_fe_batch(cpu_en._m, None, None, o.ctypes.data_as(C.c_void_p), 2, None,
                                fo.ctypes.data_as(C.c_void_p), None) == -1
        assert "ssw_fe_batch" in _lib.last_error()
    o = np.array([0, 10], np.int64)
    assert lib.ssw_fe_batch(cpu_en._m, None, None, None, 1, None, fo.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.ssw_fe_batch(cpu_en._m, None, None, o.ctypes.data_as(C.c_void_p), 1, None, None, None) == -1
    assert lib.ssw_fe_batch(cpu_en._m, None, None, o.ctypes.data_as(C.c_void_p), -1, None,
                            fo.ctypes.data_as(C.c_void_p), None) == -1
    assert lib.ssw_fe_batch(None, None, None, o.ctypes.data_as(C.c_void_p), 1, None,
                            fo.ctypes.data_as(C.c_void_p), None) == -1
    with pytest.raises(ssw.SswError, match="len\\(pcm\\)"):
        cpu_en.fe_batch(np.zeros(10, np.int16), samp_off=[0, 5])
    with pytest.raises(ssw.SswError, match="unknown"):
        cpu_en.fe_config(transform="mfcc")
    with pytest.raises(ssw.SswError, match="unknown"):
        cpu_en.fe_config(sample_rate=16000)
    # frames to compute and no device: refused, no CPU fallback
    with pytest.raises(ssw.SswError, match="no GPU"):
        cpu_en.fe_batch(np.zeros(1000, np.int16))


def test_empty_batches_need_no_device(cpu_en):
    cep, fo = cpu_en.fe_batch([np.zeros(0, np.int16), np.zeros(0, np.int16)])
    assert cep.shape == (0, 13) and list(fo) == [0, 0, 0]
    cep, fo = cpu_en.fe_batch(np.zeros(0, np.int16))
    assert cep.shape == (0, 13) and list(fo) == [0, 0]
