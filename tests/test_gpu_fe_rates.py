"""The front end at each utterance's own sample rate on the GPU (ssw_fe_batch_ex, K8's spectrum
kernel at 64 .. 8192 points) against the reference library's own cepstra and alignments, recorded
in tests/golden/fe_rates_mfcc.npz and fe_rates_align.json (tests/golden/make_mfcc_rates.py).
Every comparison of cepstra is tobytes() equality."""
import json

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fe_rates_common as R
from tests.test_gpu_fe import _params, _raw, _same, _same_alignment
from tests.test_gpu_first_pass import _lex

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(R.MFCC_NPZ)


@pytest.mark.parametrize("fx", R.FIXTURES, ids=[f[0] for f in R.FIXTURES])
def test_fixture(gpu_en, gold, fx):
    name, rate, cfg, spec = fx
    pcm = R.fixture_pcm(spec, rate)
    want = gold["cep/" + name]
    cep, fo = gpu_en.fe_batch_rates(pcm, rate, cfg=cfg)
    assert list(fo) == [0, len(want)]
    _same(cep, want, name)
    d_cep, fo2 = gpu_en.fe_batch_rates_device(torch.from_numpy(pcm).cuda(), [0, len(pcm)], rate,
                                              cfg=cfg)
    assert list(fo2) == [0, len(want)]
    _same(d_cep.cpu().numpy(), want, name + " (device)")


def test_16khz_equals_fe_batch_on_a_ragged_batch(gpu_en):
    rng = np.random.default_rng(11)
    go, fr = _raw("goforward.raw"), _raw("goforward_fr.raw")
    pcms = [go[:k] for k in (1, 409, 410, 411, 569)]
    pcms += [np.zeros(0, np.int16)]
    pcms += [go[1000:1000 + k] for k in (570, 571)] + [go]
    pcms += [np.zeros(5000, np.int16),
             np.where(rng.random(7000) < 0.5, 32767, -32768).astype(np.int16),
             rng.integers(-32768, 32768, 3000).astype(np.int16),
             (go.astype(np.int32) * 3).clip(-32768, 32767).astype(np.int16),
             (go // 7).astype(np.int16), (go.astype(np.int32) + 900).clip(-32768, 32767).astype(np.int16),
             fr[::2].copy(), -fr]
    for cfg in (None, dict(transform="legacy", remove_noise=False, lifter=0, nfilt=40,
                           lowerf=133.33334, upperf=6855.4976)):
        want, wfo = gpu_en.fe_batch(pcms, cfg=cfg)
        got, gfo = gpu_en.fe_batch_rates(pcms, 16000, cfg=cfg)
        assert list(gfo) == list(wfo)
        _same(got, want, "16 kHz")
        got, gfo = gpu_en.fe_batch_rates(pcms, None, cfg=cfg)     # cfg's samprate, 16000
        _same(got, want, "16 kHz, cfg's samprate")


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_mixed_rates(gpu_en, gold, order):
    rates = list(R.RATES) if order == "ascending" else list(R.RATES)[::-1]
    pcms, srs, want = [], [], []
    for k, r in enumerate(rates):
        shift, size = R.framing(r)
        pcms.append(R.resample(R.goforward(), r))
        srs.append(r)
        want.append(gold[f"cep/rate{r}"])
        # an empty utterance and one shorter than a window between them
        pcms.append(np.zeros(0, np.int16))
        srs.append(rates[(k + 3) % len(rates)])
        want.append(None)
        pcms.append(R.resample(R.goforward(), r)[5000:5000 + size - 1 - k])
        srs.append(r)
        want.append(None)
    cep, fo = gpu_en.fe_batch_rates(pcms, srs)
    assert list(np.diff(fo)) == list(ssw.fe_frame_counts_at([len(p) for p in pcms], srs))
    for u, (p, r, w) in enumerate(zip(pcms, srs, want)):
        mine = cep[fo[u]:fo[u + 1]]
        if w is not None:
            _same(mine, w, f"utterance {u} at {r} Hz")
        alone, _ = gpu_en.fe_batch_rates(p, r)
        _same(mine, alone, f"utterance {u} at {r} Hz alone")


def _align_batch(gpu, lex, rate, active):
    pcm = R.resample(R.goforward(), rate)
    texts = [R.ALIGN_TEXT.split()]
    aset = ssw.align_audio_batch(gpu, lex, pcm, [0, len(pcm)], texts, active=active, samprate=rate)
    # the same from the cepstra of fe_batch_rates through feat_batch and align_text_batch
    cep, fo = gpu.fe_batch_rates(pcm, rate)
    d_feats = torch.from_numpy(gpu.feat_batch(cep, utt_off=fo)).cuda()
    fn = ssw.align_text_batch_active if active else ssw.align_text_batch
    want = fn(gpu, lex, d_feats, fo, texts)
    return aset, want


@pytest.mark.parametrize("rate", R.ALIGN_RATES)
@pytest.mark.parametrize("active", [False, True])
def test_audio_to_alignment(gpu_en, rate, active):
    ref = json.load(open(R.ALIGN_JSON))[f"{rate}/{'no' if active else 'yes'}"]
    lex = _lex(gpu_en, "en-us")
    aset, want = _align_batch(gpu_en, lex, rate, active)
    assert aset.status(0) == want.status(0) == 0
    _same_alignment(aset, want, 0)
    assert aset.json(0) == ref
    aset.free()
    want.free()
    lex.free()


def test_kernel_timing_covers_every_launch(gpu_en):
    pcms = [R.resample(R.goforward(), r) for r in (16000, 44100, 8000)]
    gpu_en.set_kernel_timing(True)
    try:
        gpu_en.fe_batch_rates(pcms, [16000, 44100, 8000])
        ms = gpu_en.fe_kernel_timing()
    finally:
        gpu_en.set_kernel_timing(False)
    assert len(ms) == 3 and all(t > 0 for t in ms)


def test_feat_params_default_unchanged(gpu_en):
    """fe_batch still takes only 16 kHz; the model's own settings give the recorded cepstra"""
    with pytest.raises(ssw.SswError, match="samprate"):
        gpu_en.fe_batch(_raw("goforward.raw"), cfg={"samprate": 44100.0})
    assert _params("en-us")["nfilt"] == 20
