"""float32 audio, host side (no GPU): ssw_fe_batch_f32 without a device checks its arguments and
writes frame_off_out like ssw_fe_batch_ex; the Python helpers choose the entry point by dtype and
refuse the dtypes that used to be cut to integers or read as something they are not; the float
inputs of tests/inputs_common.py are what they say; and (where build() made the reference
library) the committed fixtures are what the reference makes.

test_f32_entry_*, test_dtype_* and test_list_* need the feature; the others pin the inputs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from soundswallower_amd.api import _pcm_kind
from tests import fe_rates_common as R
from tests import inputs_common as I
from tests.conftest import MODEL_ROOT, ROOT


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def cpu_en(lib):
    return ssw.Model(os.path.join(MODEL_ROOT, "en-us"), config={"device": ssw.SSW_DEVICE_NONE})


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_f32_entry_writes_frame_offsets_then_needs_a_device(lib, cpu_en):
    off = np.array([0, 1000, 2000, 2000, 3000], np.int64)
    rates = np.array([16000.0, 44100.0, 8000.0, 8000.0])
    for fn in (lib.ssw_fe_batch_f32, lib.ssw_fe_batch_ex):
        fo = np.full(5, 77, np.int32)
        assert fn(cpu_en._m, None, None, _p(off), _p(rates), 4, None, _p(fo), None) == -1
        assert "no GPU" in _lib.last_error()
        assert list(np.diff(fo)) == list(ssw.fe_frame_counts_at(np.diff(off), rates))
    # samprate NULL: the configuration's rate for every utterance
    fo = np.full(5, 77, np.int32)
    assert lib.ssw_fe_batch_f32(cpu_en._m, None, None, _p(off), None, 4, None, _p(fo), None) == -1
    assert list(np.diff(fo)) == list(ssw.fe_frame_counts(np.diff(off)))
    # no samples: nothing to do, no device needed
    off0 = np.zeros(3, np.int64)
    fo = np.full(3, 77, np.int32)
    assert lib.ssw_fe_batch_f32(cpu_en._m, None, None, _p(off0), None, 2, None, _p(fo), None) == 0
    assert list(fo) == [0, 0, 0]


def test_f32_entry_refuses_what_the_int16_entry_refuses(lib, cpu_en):
    off = np.array([0, 1000, 2000, 3000], np.int64)
    fo = np.full(4, 77, np.int32)
    for bad in (16000.25, 0.5, 1e12, float("nan")):
        rates = np.array([16000.0, 44100.0, bad])
        msgs = []
        for fn in (lib.ssw_fe_batch_f32, lib.ssw_fe_batch_ex):
            assert fn(cpu_en._m, None, None, _p(off), _p(rates), 3, None, _p(fo), None) == -1
            msgs.append(_lib.last_error())
            assert list(fo) == [77] * 4
        assert "utterance 2" in msgs[0]
        assert msgs[0] == msgs[1].replace("ssw_fe_batch_ex", "ssw_fe_batch_f32")
    bad_off = np.array([0, 1000, 500, 3000], np.int64)
    assert lib.ssw_fe_batch_f32(cpu_en._m, None, None, _p(bad_off), None, 3, None, _p(fo), None) == -1
    assert "samp_off decreases at utterance 1" in _lib.last_error()
    for args in ((None, None, None, _p(off), None, 3, None, _p(fo), None),
                 (cpu_en._m, None, None, None, None, 3, None, _p(fo), None),
                 (cpu_en._m, None, None, _p(off), None, 3, None, None, None),
                 (cpu_en._m, None, None, _p(off), None, -1, None, _p(fo), None),
                 (cpu_en._m, None, None, _p(off[1:]), None, 2, None, _p(fo), None)):
        assert lib.ssw_fe_batch_f32(*args) == -1
        assert "bad arguments to ssw_fe_batch_f32" in _lib.last_error()
    assert list(fo) == [77] * 4


@pytest.mark.parametrize("over,msg", [
    ({"transform": "htk"}, "htk"), ({"dither": 1}, "dither"), ({"ncep": 12}, "ncep"),
    ({"alpha": 0.95}, "alpha"), ({"nfft": 256}, "nfft 256"), ({"frate": 0}, "frate")])
def test_f32_settings_refused_as_for_int16(cpu_en, over, msg):
    for pcm in (np.zeros(1000, np.float32), np.zeros(1000, np.int16)):
        with pytest.raises(ssw.SswError, match=msg):
            cpu_en.fe_batch_rates(pcm, 16000, cfg=over)


def test_dtype_picks_the_entry_point(cpu_en):
    with pytest.raises(ssw.SswError, match="^ssw_fe_batch_f32: .*no GPU"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.float32), 44100)
    with pytest.raises(ssw.SswError, match="^ssw_fe_batch_f32: .*no GPU"):
        cpu_en.fe_batch(np.zeros(1000, np.float32))
    with pytest.raises(ssw.SswError, match="^ssw_fe_batch_ex: .*no GPU"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int16), 44100)
    with pytest.raises(ssw.SswError, match="^ssw_fe_batch: .*no GPU"):
        cpu_en.fe_batch(np.zeros(1000, np.int16))
    with pytest.raises(ssw.SswError, match="^ssw_fe_batch_ex: .*no GPU"):
        cpu_en.fe_batch_rates(np.zeros(1000, np.int32), 44100)      # integer dtypes as before
    cep, fo = cpu_en.fe_batch_rates([np.zeros(0, np.float32)] * 2, [44100, 8000])
    assert cep.shape == (0, 13) and list(fo) == [0, 0, 0]
    assert _pcm_kind(np.zeros(3, np.float32)) == "f32"
    assert _pcm_kind(np.zeros(3, np.int16)) == _pcm_kind(np.zeros(3, np.uint8)) == "i16"
    assert _pcm_kind([1, 2, 3]) == "i16"
    # a raw device pointer stays int16 unless it is said to be float32
    assert _pcm_kind(12345) == "i16" and _pcm_kind(12345, "f32") == "f32"
    assert _pcm_kind(None) == "i16"
    with pytest.raises(ssw.SswError, match="pcm_format"):
        _pcm_kind(12345, "f64")
    with pytest.raises(ssw.SswError, match="pcm_format 'f32' given for i16 audio"):
        _pcm_kind(np.zeros(3, np.int16), "f32")


@pytest.mark.parametrize("dtype", [np.float64, np.float16, np.complex64])
def test_dtype_that_was_silently_cut_is_refused_by_name(cpu_en, dtype):
    x = np.zeros(1000, dtype)
    for call in (lambda: cpu_en.fe_batch(x), lambda: cpu_en.fe_batch_rates(x, 16000),
                 lambda: cpu_en.fe_batch([x, x]),
                 lambda: ssw.align_audio_batch(cpu_en, None, x, [0, 1000], [["go"]]),
                 lambda: ssw.recognize_audio_batch(cpu_en, None, x, [0, 1000], None),
                 lambda: ssw.recognize_align_audio_batch(cpu_en, None, x, [0, 1000], None)):
        with pytest.raises(ssw.SswError, match=np.dtype(dtype).name):
            call()


def test_dtype_of_a_tensor():
    torch = pytest.importorskip("torch")
    assert _pcm_kind(torch.zeros(3, dtype=torch.float32)) == "f32"      # on the host: as an array
    assert _pcm_kind(torch.zeros(3, dtype=torch.int16)) == "i16"
    for dt in (torch.float64, torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(ssw.SswError, match=str(dt).replace("torch.", "")):
            _pcm_kind(torch.zeros(3, dtype=dt))


def test_list_must_be_all_one_kind(cpu_en):
    with pytest.raises(ssw.SswError, match="all int16 or all float32"):
        cpu_en.fe_batch_rates([np.zeros(10, np.float32), np.zeros(10, np.int16)], 16000)
    with pytest.raises(ssw.SswError, match="float64"):
        cpu_en.fe_batch_rates([np.zeros(10, np.float32), np.zeros(10, np.float64)], 16000)


def test_float_inputs_are_what_they_say():
    x = I.int_pcm(16000)
    assert np.array_equal(I.f32_pcm("exact", 16000) * np.float32(32768), x.astype(np.float32))
    assert np.abs(I.f32_pcm("loud", 16000)).max() > 3.0 > 1.0 > np.abs(I.f32_pcm("beyond", 16000)).max()
    tiny = I.f32_pcm("tiny", 16000)
    assert 0 < np.abs(tiny[tiny != 0]).min() == 2.0 ** -40
    frac = I.f32_pcm("frac", 16000) * np.float32(32768)
    assert np.any(frac != np.round(frac))
    assert not I.f32_pcm("zero", 44100, 441).any() and len(I.f32_pcm("zero", 44100, 441)) == 441
    assert I.edge_lengths(16000) == (1, 409, 410, 411, 569, 570, 571)
    assert I.edge_lengths(44100) == (1, 1129, 1130, 1131, 1570, 1571, 1572)
    gold = np.load(I.F32_NPZ)
    assert sorted(gold.files) == sorted(
        ["cep/" + f[0] for f in I.FE_FIXTURES]
        + [I.align_key(k, r, c) for k, r in I.ALIGN_CASES for c in I.CONFIGS])
    # the reference's own cepstra of x / 32768 are those of the int16 audio
    rates = np.load(R.MFCC_NPZ)
    # (the full frames of the 1 s piece: its last frame is fe_end's, of other samples)
    full = 1 + (44100 - R.framing(44100)[1]) // R.framing(44100)[0]
    assert gold["cep/exact_44100"][:full].tobytes() == rates["cep/rate44100"][:full].tobytes()
    for name, kind, rate, cfg, n in I.FE_FIXTURES:
        assert len(gold["cep/" + name]) == ssw.fe_frame_counts_at([n], rate)[0], name
    assert os.path.getsize(I.F32_NPZ) < os.path.getsize(R.MFCC_NPZ) // 2


@pytest.mark.skipif(not reference.available(),
                    reason="no reference build in oracle/_ref/: build() makes it when it finds a "
                           "SoundSwallower source tree (oracle/reference.py)")
def test_fixtures_are_what_the_reference_makes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_inputs.py"),
                        "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
