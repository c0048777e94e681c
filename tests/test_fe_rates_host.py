"""The front end at any sample rate, host side (no GPU): ssw_fe_frame_count_ex and
fe_frame_counts_at against the reference's recorded frame counts, the settings ssw_fe_batch_ex
refuses and why, samprate 0, and (where build() made the reference library) that the committed
fixtures are what the reference makes."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from tests import fe_rates_common as R
from tests.conftest import MODEL_ROOT, ROOT


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cpu_en(lib):
    return ssw.Model(os.path.join(MODEL_ROOT, "en-us"), config={"device": -2})


def test_frame_counts_match_the_reference(lib, cpu_en):
    gold = np.load(R.MFCC_NPZ)
    for rate in R.RATES:
        want = gold[f"counts/{rate}"]
        n = np.arange(1, len(want) + 1)
        assert len(want) == R.count_limit(rate)
        assert list(ssw.fe_frame_counts_at(n, rate)) == list(want), rate
        assert list(cpu_en.fe_frame_counts_rates(n, rate)) == list(want), rate
        for k in (1, 100000):
            want_k = int(ssw.fe_frame_counts_at([k], rate)[0])
            assert lib.ssw_fe_frame_count_ex(cpu_en._m, None, float(rate), k) == want_k
    # one rate per utterance; 0 samples make no frame
    n = np.array([0, 44580, 44580, 1130, 1129])
    assert list(ssw.fe_frame_counts_at(n, [8000, 8000, 44100, 44100, 44100])) == \
        [0, 2 + (44580 - 205) // 80, 2 + (44580 - 1130) // 441, 2, 1]
    assert lib.ssw_fe_frame_count_ex(cpu_en._m, None, 44100.0, 0) == 0
    assert lib.ssw_fe_frame_count_ex(cpu_en._m, None, 44100.0, -1) == -1
    assert lib.ssw_fe_frame_count_ex(None, None, 44100.0, 10) == -1


def test_frame_counts_of_the_fixtures(cpu_en):
    gold = np.load(R.MFCC_NPZ)
    for name, rate, cfg, spec in R.FIXTURES:
        n = len(R.fixture_pcm(spec, rate))
        s = R.settings(cfg)
        want = len(gold["cep/" + name])
        assert cpu_en.fe_frame_counts_rates([n], rate, cfg=cfg)[0] == want, name
        assert ssw.fe_frame_counts_at([n], rate, frate=s.get("frate", 100),
                                      wlen=s.get("wlen", 0.025625))[0] == want, name


def test_frame_size_equal_to_shift(cpu_en):
    """size == shift: fe_end's frame only when samples are left over"""
    cfg = {"frate": 100, "wlen": 0.01}                                 # 80 / 80 at 8 kHz
    got = cpu_en.fe_frame_counts_rates([79, 80, 159, 160, 161], 8000, cfg=cfg)
    assert list(got) == [1, 1, 2, 2, 3]
    assert list(ssw.fe_frame_counts_at([79, 80, 159, 160, 161], 8000, wlen=0.01)) == [1, 1, 2, 2, 3]


@pytest.mark.parametrize("rate,over,msg", [
    (44100.5, {}, "whole number"),
    (-8000.0, {}, "whole number"),
    (8000, {"frate": 0}, "frate"),
    (8000, {"frate": 8001}, "frate"),
    (48000, {"frate": 40000}, "frate"),
    (8000, {"frate": 6000, "wlen": 0.01}, "shift 1 "),
    (16000, {"frate": 50, "wlen": 0.01}, "frame size 160 .*shift 320"),
    (44100, {"nfft": 1024}, "nfft 1024 is smaller"),
    (44100, {"nfft": 3000}, "power of 2"),
    (16000, {"nfft": 256}, "nfft 256"),
    (192000, {"wlen": 0.05}, "8192"),
    (96000, {"wlen": 0.2}, "8192"),
    (8000, {"wlen": 0.004, "frate": 400}, "32-point FFT .* 64 .. 8192"),
    (8000, {"upperf": 4001.5}, "upperf"),
    (16000, {"upperf": 8002.0}, "upperf"),
])
def test_refusals(cpu_en, rate, over, msg):
    with pytest.raises(ssw.SswError, match=msg):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), rate, cfg=over)
    with pytest.raises(ssw.SswError, match=msg):
        cpu_en.fe_frame_counts_rates([1000], rate, cfg=over)


def test_narrow_filters_are_refused(cpu_en):
    """20 filters at a 64-point FFT: narrower than one DFT point (the reference's cepstra are
    NaN); 5 filters are fine and need a device"""
    small = {"wlen": 0.008, "frate": 200, "lowerf": 130.0, "upperf": 3700.0}
    with pytest.raises(ssw.SswError, match="narrower than one DFT point"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), 8000, cfg=dict(small, nfilt=20))
    with pytest.raises(ssw.SswError, match="no GPU"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), 8000, cfg=dict(small, nfilt=5))


def test_upperf_rule_has_the_references_plus_one(cpu_en):
    with pytest.raises(ssw.SswError, match="no GPU"):                  # accepted, needs a GPU
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), 8000, cfg={"upperf": 4001.0})
    with pytest.raises(ssw.SswError, match="upperf <= samprate / 2"):  # ssw_fe_batch: unchanged
        cpu_en.fe_batch(np.zeros(1000, np.int16), cfg={"upperf": 8001.0})
    with pytest.raises(ssw.SswError, match="no GPU"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), 16000, cfg={"upperf": 8001.0})


def test_one_bad_rate_refuses_the_call_and_writes_nothing(lib, cpu_en):
    off = np.array([0, 1000, 2000, 3000], np.int64)
    fo = np.full(4, 77, np.int32)
    for bad in (16000.25, 0.5, 1e12, float("nan")):
        rates = np.array([16000.0, 44100.0, bad])
        assert lib.ssw_fe_batch_ex(cpu_en._m, None, None, off.ctypes.data_as(C.c_void_p),
                                   rates.ctypes.data_as(C.c_void_p), 3, None,
                                   fo.ctypes.data_as(C.c_void_p), None) == -1
        assert "utterance 2" in _lib.last_error()
        assert list(fo) == [77] * 4
    # good rates: frame offsets written, then no device
    rates = np.array([16000.0, 44100.0, 8000.0])
    assert lib.ssw_fe_batch_ex(cpu_en._m, None, None, off.ctypes.data_as(C.c_void_p),
                               rates.ctypes.data_as(C.c_void_p), 3, None,
                               fo.ctypes.data_as(C.c_void_p), None) == -1
    assert "no GPU" in _lib.last_error()
    assert list(np.diff(fo)) == list(ssw.fe_frame_counts_at([1000] * 3, rates))


def test_samprate_zero_picks_the_minimum_rate(tmp_path, cpu_en):
    # en-us: upperf 3700 -> 8000
    assert cpu_en.fe_frame_counts_rates([1000], 0)[0] == ssw.fe_frame_counts_at([1000], 8000)[0]
    assert cpu_en.fe_frame_counts_rates([1000], None, cfg={"samprate": 0})[0] == \
        ssw.fe_frame_counts_at([1000], 8000)[0]
    # the reference defaults: upperf 6855.4976 -> 16000
    src = os.path.join(MODEL_ROOT, "en-us")
    for f in ("mdef", "means", "variances", "sendump", "transition_matrices"):
        os.symlink(os.path.join(src, f), tmp_path / f)
    m = ssw.Model(str(tmp_path), config={"device": -2})
    assert m.fe_frame_counts_rates([1000], 0)[0] == ssw.fe_frame_counts_at([1000], 16000)[0] == 5


def test_model_with_an_8khz_feat_params(tmp_path):
    src = os.path.join(MODEL_ROOT, "en-us")
    for f in ("mdef", "means", "variances", "sendump", "transition_matrices"):
        os.symlink(os.path.join(src, f), tmp_path / f)
    p = json.load(open(os.path.join(src, "feat_params.json")))
    p["samprate"] = 8000
    (tmp_path / "feat_params.json").write_text(json.dumps(p))
    m = ssw.Model(str(tmp_path), config={"device": -2})
    assert m.fe_config().samprate == 8000
    # ssw_fe_batch refuses it, as before; _ex takes it with no overrides
    with pytest.raises(ssw.SswError, match="samprate 16000"):
        m.fe_batch(np.zeros(1000, np.int16))
    with pytest.raises(ssw.SswError, match="no GPU"):
        m.fe_batch_rates(np.zeros(1000, np.int16), None)
    assert m.fe_frame_counts_rates([1000])[0] == ssw.fe_frame_counts_at([1000], 8000)[0]


@pytest.mark.parametrize("over,msg", [
    ({"transform": "htk"}, "htk"), ({"dither": 1}, "dither"), ({"remove_dc": 1}, "remove_dc"),
    ({"smoothspec": 1}, "smoothspec"), ({"logspec": 1}, "logspec"), ({"warp": 1}, "warp"),
    ({"doublebw": 1}, "doublebw"), ({"ncep": 12}, "ncep"), ({"alpha": 0.95}, "alpha"),
    ({"nfilt": 65}, "nfilt"), ({"nfilt": 0}, "nfilt"), ({"lifter": -1}, "lifter"),
    ({"lowerf": 4000.0, "upperf": 3000.0}, "lowerf"), ({"lowerf": -1.0}, "lowerf"),
    ({"unit_area": 0}, "unit_area"), ({"round_filters": 0}, "round_filters")])
def test_settings_refused_as_by_fe_batch(cpu_en, over, msg):
    for rate in (44100, 16000):
        with pytest.raises(ssw.SswError, match=msg):
            cpu_en.fe_batch_rates(np.zeros(1000, np.int16), rate, cfg=over)


def test_empty_batches_need_no_device(cpu_en):
    cep, fo = cpu_en.fe_batch_rates([np.zeros(0, np.int16)] * 2, [44100, 8000])
    assert cep.shape == (0, 13) and list(fo) == [0, 0, 0]


def test_resampling_is_integer_only():
    x = R.goforward()
    assert np.array_equal(R.resample(x, 16000), x)
    y = R.resample(x, 44100)
    assert len(y) == len(x) * 44100 // 16000 and y.dtype == np.int16
    i, r = divmod(1001 * 16000, 44100)
    assert y[1001] == (int(x[i]) * (44100 - r) + int(x[i + 1]) * r) // 44100


@pytest.mark.skipif(not reference.available(),
                    reason="no reference build in oracle/_ref/: build() makes it when it finds a "
                           "SoundSwallower source tree (oracle/reference.py)")
def test_fixtures_are_what_the_reference_makes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_mfcc_rates.py"),
                        "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
