"""The front end under the settings only ssw_fe_batch_any takes (remove_dc, any alpha, htk, any
ncep, logspec, smoothspec, doublebw, unit_area, round_filters, frequency warping) on the GPU
against the reference library's own rows and alignments, recorded in tests/golden/fe_any_mfcc.npz
and fe_any_align.json (tests/golden/make_fe_any.py).  Every comparison of rows is tobytes()
equality."""
import json

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fe_any_common as A
from tests import fe_rates_common as R
from tests.test_gpu_fe import _raw, _same, _same_alignment
from tests.test_gpu_first_pass import _lex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(A.MFCC_NPZ)


def _fe(gpu, cfg):
    s, warp_type, warp_params = A.settings(cfg)
    return gpu.fe(s, warp_type, warp_params)


@pytest.mark.parametrize("fx", A.FIXTURES, ids=[f[0] for f in A.FIXTURES])
def test_fixture(gpu_en, gold, fx):
    name, rate, cfg, _, _ = fx
    pcm = A.fixture_pcm(fx)
    want = gold["cep/" + name]
    fe = _fe(gpu_en, cfg)
    assert fe.out_dim == want.shape[1]
    rows, fo = gpu_en.fe_batch_any(pcm, rate, fe)
    assert list(fo) == [0, len(want)]
    _same(rows, want, name)
    d_rows, fo2 = gpu_en.fe_batch_any_device(torch.from_numpy(pcm).cuda(), [0, len(pcm)], rate,
                                             fe=fe)
    assert list(fo2) == [0, len(want)]
    _same(d_rows.cpu().numpy(), want, name + " (device)")
    fe.free()


def test_float32_of_int16_audio_gives_the_int16_bytes(gold):
    assert gold["cep/dc_f32_exact"].tobytes() == gold["cep/remove_dc"].tobytes()


def test_a_plain_configuration_gives_the_older_entry_points_bytes(gpu_en):
    rng = np.random.default_rng(11)
    go, fr = _raw("goforward.raw"), _raw("goforward_fr.raw")
    pcms = [go[:k] for k in (1, 409, 410, 411, 569)]
    pcms += [np.zeros(0, np.int16)]
    pcms += [go[1000:1000 + k] for k in (570, 571)] + [go[:20000]]
    pcms += [np.where(rng.random(3000) < 0.5, 32767, -32768).astype(np.int16),
             rng.integers(-32768, 32768, 3000).astype(np.int16), fr[:9000:2].copy()]
    rates = [16000, 22050, 44100] * 4
    for cfg in (None, dict(transform="legacy", remove_noise=False, lifter=0, nfilt=40,
                           lowerf=133.33334, upperf=6855.4976)):
        fe = gpu_en.fe(cfg)
        want, wfo = gpu_en.fe_batch_rates(pcms, rates, cfg=cfg)
        got, gfo = gpu_en.fe_batch_any(pcms, rates, fe)
        assert list(gfo) == list(wfo)
        _same(got, want, "int16")
        f32 = [p.astype(np.float32) / np.float32(3 * 32768) for p in pcms]
        want, wfo = gpu_en.fe_batch_rates(f32, rates, cfg=cfg)
        got, gfo = gpu_en.fe_batch_any(f32, rates, fe)
        assert list(gfo) == list(wfo)
        _same(got, want, "float32")
        fe.free()


@pytest.mark.parametrize("order", ["8000 first", "44100 first"])
def test_mixed_rates_with_remove_dc(gpu_en, order):
    """one batch of 8000 Hz and 44100 Hz utterances (two FFT sizes, one launch each); every
    utterance's rows are those of the utterance alone"""
    fe = _fe(gpu_en, {"remove_dc": True})
    rates = [8000, 44100, 8000, 44100, 44100, 8000]
    if order == "44100 first":
        rates = rates[::-1]
    pcms = [R.resample(R.goforward(), r)[1000 * k:1000 * k + int(0.3 * r) + 7 * k]
            for k, r in enumerate(rates)]
    pcms[2] = pcms[2][:0]
    pcms[3] = pcms[3][:100]                              # shorter than a window
    rows, fo = gpu_en.fe_batch_any(pcms, rates, fe)
    assert list(np.diff(fo)) == [int(fe.frames(len(p), r)) for p, r in zip(pcms, rates)]
    for u, (p, r) in enumerate(zip(pcms, rates)):
        alone, _ = gpu_en.fe_batch_any(p, r, fe)
        _same(rows[fo[u]:fo[u + 1]], alone, f"utterance {u} at {r} Hz")
    # and at 16 kHz the recorded rows, in a batch with other rates around them
    fx = next(f for f in A.FIXTURES if f[0] == "remove_dc")
    rows, fo = gpu_en.fe_batch_any([pcms[0], A.fixture_pcm(fx), pcms[1]],
                                   [rates[0], 16000, rates[1]], fe)
    _same(rows[fo[1]:fo[2]], np.load(A.MFCC_NPZ)["cep/remove_dc"], "16 kHz among other rates")
    fe.free()


@pytest.fixture(scope="module")
def changed(tmp_path_factory):
    """en-us with remove_dc, round_filters = no and alpha 0.95 in its feat_params.json"""
    m = ssw.Model(A.align_model_dir(str(tmp_path_factory.mktemp("fe_any") / "en-us-changed")))
    yield m
    m.close()


@pytest.mark.parametrize("active", [False, True])
def test_audio_to_alignment_under_the_models_own_settings(changed, active):
    ref = json.load(open(A.ALIGN_JSON))["no" if active else "yes"]
    assert not changed.fe_plain()
    lex = _lex(changed, "en-us")
    pcm = R.goforward()
    texts = [A.ALIGN_TEXT.split()]
    aset = ssw.align_audio_batch(changed, lex, pcm, [0, len(pcm)], texts, active=active)
    # the same from the rows of fe_batch_any through feat_batch and align_text_batch
    rows, fo = changed.fe_batch_any(pcm)
    d_feats = torch.from_numpy(changed.feat_batch(rows, utt_off=fo)).cuda()
    fn = ssw.align_text_batch_active if active else ssw.align_text_batch
    want = fn(changed, lex, d_feats, fo, texts)
    assert aset.status(0) == want.status(0) == 0
    _same_alignment(aset, want, 0)
    assert aset.json(0) == ref
    # a dict of settings keeps the older route, which refuses remove_dc by name
    with pytest.raises(ssw.SswError, match="remove_dc is not supported"):
        ssw.align_audio_batch(changed, lex, pcm, [0, len(pcm)], texts, active=active, fe_cfg={})
    aset.free()
    want.free()
    lex.free()


def test_a_model_with_plain_settings_takes_the_old_route(gpu_en, monkeypatch):
    assert gpu_en.fe_plain()
    calls = []
    real = gpu_en.fe_batch_any_device
    monkeypatch.setattr(gpu_en, "fe_batch_any_device",
                        lambda *a, **k: calls.append(1) or real(*a, **k))
    lex = _lex(gpu_en, "en-us")
    pcm = R.goforward()
    texts = [A.ALIGN_TEXT.split()]
    aset = ssw.align_audio_batch(gpu_en, lex, pcm, [0, len(pcm)], texts)
    assert aset.status(0) == 0 and not calls
    # an Fe of the caller's goes through the new entry, and a plain one gives the same alignment
    fe = gpu_en.fe()
    other = ssw.align_audio_batch(gpu_en, lex, pcm, [0, len(pcm)], texts, fe_cfg=fe)
    assert calls and other.json(0) == aset.json(0)
    fe.free()
    aset.free()
    other.free()
    lex.free()


def test_kernel_timing_covers_the_new_launches(gpu_en):
    fe = _fe(gpu_en, {"remove_dc": True, "ncep": 20})
    pcms = [R.resample(R.goforward(), r)[:r] for r in (16000, 44100)]
    gpu_en.set_kernel_timing(True)
    try:
        gpu_en.fe_batch_any(pcms, [16000, 44100], fe)
        ms = gpu_en.fe_kernel_timing()
    finally:
        gpu_en.set_kernel_timing(False)
    assert len(ms) == 3 and all(t > 0 for t in ms)
    fe.free()
