"""The MFCC front end on the GPU (ssw_fe_batch, K8) against the oracle's restatement of the
reference's front end (oracle/ssw_oracle_fe.c: fe_process_int16 + fe_end over whole
utterances), byte for byte, and audio + text -> alignment in one batch (align_audio_batch)
against the reference's recorded outputs.  Every comparison of cepstra is tobytes() equality."""
import json
import math
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests.conftest import MODEL_ROOT, ROOT
from tests.test_gpu_first_pass import _lex
from tests.test_reference_pins import REF_FR_TEXTS, parse_words

pytestmark = pytest.mark.gpu

GOLD = os.path.join(ROOT, "tests", "golden")


def _raw(name):
    return np.fromfile(os.path.join(GOLD, name), dtype="<i2")


def _params(name):
    p = json.load(open(os.path.join(MODEL_ROOT, name, "feat_params.json")))
    return dict(nfilt=p["nfilt"], lowerf=p["lowerf"], upperf=p["upperf"], lifter=p["lifter"],
                remove_noise=p["remove_noise"], transform=p["transform"])


def _oracle(O, pcm, nfilt=40, lowerf=133.33334, upperf=6855.4976, lifter=0, remove_noise=False,
            transform="legacy"):
    """the oracle's cepstra; the lifter after the legacy transform as the reference applies it
    (fe_write_frame -> fe_lifter after fe_mel_cep whatever the transform, src/fe_sigproc.c:
    701-738; the oracle's legacy branch returns before it, which matters only for lifter != 0)"""
    cep = O.fe_mfcc(pcm, nfilt=nfilt, lowerf=lowerf, upperf=upperf, lifter=lifter,
                    remove_noise=remove_noise, transform=transform)
    if transform == "legacy" and lifter:
        lift = np.array([np.float32(1 + lifter // 2 * math.sin(i * math.pi / lifter))
                         for i in range(13)], np.float32)
        cep = (cep * lift).astype(np.float32)
    return cep


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        f, i = bad[0]
        pytest.fail(f"{what}: {len(bad)} values differ, first frame {f} cep {i}: "
                    f"{got[f, i]!r} vs {want[f, i]!r}")


def _check_batch(O, gpu, pcms, cfg=None, **oc):
    cep, fo = gpu.fe_batch(pcms, cfg=cfg)
    assert list(np.diff(fo)) == [int(ssw.fe_frame_counts([len(p)])[0]) for p in pcms]
    for u, p in enumerate(pcms):
        _same(cep[fo[u]:fo[u + 1]], _oracle(O, p, **oc), f"utterance {u} ({len(p)} samples)")
    return cep, fo


@pytest.mark.parametrize("name,raw,gold,n", [
    ("en-us", "goforward.raw", "goforward_mfcc.npy", 278),
    ("fr-fr", "goforward_fr.raw", "goforward_fr_mfcc.npy", 239)])
def test_goldens(oracle_mod, gpu_en, gpu_fr, name, raw, gold, n):
    gpu = gpu_en if name == "en-us" else gpu_fr
    pcm = _raw(raw)
    cep, fo = gpu.fe_batch(pcm)                           # feat_params.json's settings
    assert list(fo) == [0, n]
    _same(cep, np.load(os.path.join(GOLD, gold)).astype(np.float32), gold)
    _same(cep, _oracle(oracle_mod, pcm, **_params(name)), "oracle")
    # the same from device memory, into a tensor the call allocates
    d_cep, fo2 = gpu.fe_batch_device(torch.from_numpy(pcm.copy()).cuda(), [0, len(pcm)])
    assert list(fo2) == [0, n]
    _same(d_cep.cpu().numpy(), cep, "fe_batch_device")


def test_ragged_batch(oracle_mod, gpu_en):
    rng = np.random.default_rng(11)
    go, fr = _raw("goforward.raw"), _raw("goforward_fr.raw")
    pcms = [go[:k] for k in (1, 409, 410, 411, 569)]
    pcms += [np.zeros(0, np.int16)]                                      # 0 frames, mid-batch
    pcms += [go[1000:1000 + k] for k in (570, 571)] + [go]
    pcms += [np.zeros(5000, np.int16),                                   # silence
             np.where(rng.random(7000) < 0.5, 32767, -32768).astype(np.int16),   # clipped noise
             rng.integers(-32768, 32768, 3000).astype(np.int16),
             (go.astype(np.int32) * 3).clip(-32768, 32767).astype(np.int16),
             (go // 7).astype(np.int16), (go.astype(np.int32) + 900).clip(-32768, 32767).astype(np.int16),
             fr[::2].copy(), -fr]
    assert len(go) == 44580
    cep, fo = _check_batch(oracle_mod, gpu_en, pcms, **_params("en-us"))
    assert fo[6] - fo[5] == 0
    # an utterance alone equals the same utterance inside the batch
    for u in (0, 3, 7, 9):
        alone, _ = gpu_en.fe_batch(pcms[u])
        _same(alone, cep[fo[u]:fo[u + 1]], f"utterance {u} alone")


@pytest.mark.parametrize("transform", ["dct", "legacy"])
@pytest.mark.parametrize("remove_noise", [True, False])
@pytest.mark.parametrize("lifter", [0, 22])
@pytest.mark.parametrize("nfilt", [20, 40])
def test_configurations(oracle_mod, gpu_en, transform, remove_noise, lifter, nfilt):
    go, fr = _raw("goforward.raw"), _raw("goforward_fr.raw")
    pcms = [go[:20000], fr[3000:9000], go[30000:30450], go[:300]]
    lo, hi = (130.0, 3700.0) if nfilt == 20 else (133.33334, 6855.4976)
    cfg = dict(transform=transform, remove_noise=remove_noise, lifter=lifter, nfilt=nfilt,
               lowerf=lo, upperf=hi)
    _check_batch(oracle_mod, gpu_en, pcms, cfg=cfg, **cfg)


def test_more_filters_and_bands(oracle_mod, gpu_en):
    """nfilt up to the 64 lanes of a wave, other band edges"""
    go = _raw("goforward.raw")
    for nfilt, lo, hi in ((64, 64.0, 8000.0), (1, 300.0, 3000.0), (33, 0.0, 5000.0)):
        cfg = dict(transform="dct", remove_noise=True, lifter=22, nfilt=nfilt, lowerf=lo, upperf=hi)
        _check_batch(oracle_mod, gpu_en, [go[:12345], go[20000:]], cfg=cfg, **cfg)


def test_randomised(oracle_mod, gpu_en, gpu_fr):
    rng = np.random.default_rng(2026)
    go, fr = _raw("goforward.raw"), _raw("goforward_fr.raw")
    pcms = []
    for _ in range(72):
        src = go if rng.random() < 0.5 else fr
        n = int(rng.integers(0, 60000))
        parts, have = [], 0
        while have < n:
            a = int(rng.integers(0, len(src) - 1))
            b = min(len(src), a + int(rng.integers(1, 20000)), a + n - have)
            parts.append(src[a:b])
            have += b - a
        x = np.concatenate(parts).astype(np.float64) if parts else np.zeros(0)
        x = x * rng.uniform(0.05, 4.0) + rng.normal(0, rng.uniform(0, 300), len(x)) + rng.integers(-500, 500)
        pcms.append(np.clip(np.round(x), -32768, 32767).astype(np.int16))
    for gpu, name in ((gpu_en, "en-us"), (gpu_fr, "fr-fr")):
        _check_batch(oracle_mod, gpu, pcms, **_params(name))


def _same_alignment(a, b, u):
    x, y = a.utterance(u), b.utterance(u)
    assert (x is None) == (y is None)
    if x is not None:
        assert x["words"] == y["words"]
        for k in ("word_al", "phone_al", "state_al", "cipid"):
            assert np.array_equal(x[k], y[k]), k
        assert a.json(u) == b.json(u)


def test_audio_to_alignment_en_us(oracle_mod, gpu_en):
    from tests.test_lexicon_host import REF_JSON_PREFIX
    from tests.test_oracle_e2e_goforward import REF_WORDS, _parse_ref
    pcm = _raw("goforward.raw")
    lex = _lex(gpu_en, "en-us")
    texts = ["go forward ten meters".split(), "go forward ten meters".split()]
    pcms = np.concatenate([pcm, pcm[:6700]])            # the second one is too short for the text
    off = [0, len(pcm), len(pcms)]
    aset = ssw.align_audio_batch(gpu_en, lex, pcms, off, texts)
    assert aset.status(0) == 0 and aset.status(1) == 1
    a = aset.utterance(0)
    assert a["words"] == [w for (w, _, _, _) in REF_WORDS]
    assert [tuple(int(x) for x in r) for r in a["word_al"]] == [(s, d, sc) for (_, s, d, sc) in REF_WORDS]
    ref = _parse_ref()
    assert [tuple(int(x) for x in r) for r in a["phone_al"]] == [(r[1], r[2], r[3]) for r in ref]
    assert aset.json(0).startswith(REF_JSON_PREFIX)
    # from a device tensor: the same
    d_pcm = torch.from_numpy(pcms.copy()).cuda()
    aset2 = ssw.align_audio_batch(gpu_en, lex, d_pcm, off, texts)
    _same_alignment(aset, aset2, 0)
    # the default configuration (compallsen = no) equals align_text_batch_active on the oracle's
    # cepstra
    cep = np.concatenate([_oracle(oracle_mod, pcm, **_params("en-us")),
                          _oracle(oracle_mod, pcm[:6700], **_params("en-us"))])
    fo = np.array([0, 278, len(cep)], np.int32)
    d_feats = torch.from_numpy(gpu_en.feat_batch(cep, utt_off=fo)).cuda()
    act = ssw.align_audio_batch(gpu_en, lex, pcms, off, texts, active=True)
    want = ssw.align_text_batch_active(gpu_en, lex, d_feats, fo, texts)
    for u in range(2):
        assert act.status(u) == want.status(u)
        _same_alignment(act, want, u)
    for s in (aset, aset2, act, want):
        s.free()
    lex.free()


def test_audio_to_alignment_fr_fr(oracle_mod, gpu_fr):
    pcm = _raw("goforward_fr.raw")
    lex = _lex(gpu_fr, "fr-fr")
    texts = list(REF_FR_TEXTS)
    k = len(texts)
    pcms = np.tile(pcm, k)
    off = np.arange(k + 1, dtype=np.int64) * len(pcm)
    # first pass from the device front end: the reference's word segmentations
    d_cep, fo = gpu_fr.fe_batch_device(torch.from_numpy(pcms).cuda(), off)
    n = fo[1]
    assert n == 239 and list(fo) == [n * u for u in range(k + 1)]
    feats = gpu_fr.feat_batch(d_cep.cpu().numpy(), utt_off=fo)
    d_feats = torch.from_numpy(feats).cuda()
    d_scr = torch.empty((k * n, gpu_fr.n_sen), dtype=torch.int16, device="cuda")
    gpu_fr.score_batch_device(d_feats, k * n, fo, d_scr)
    torch.cuda.synchronize()
    segs = lex.first_pass(d_scr, fo, [t.split() for t in texts])
    for t, seg in zip(texts, segs):
        assert [(w, s, s + d - 1) for (w, s, d, _) in seg] == parse_words(REF_FR_TEXTS[t]), t
    # audio + text -> alignments, equal to the same call from the oracle's cepstra
    aset = ssw.align_audio_batch(gpu_fr, lex, pcms, off, [t.split() for t in texts])
    cep = np.tile(_oracle(oracle_mod, pcm, **_params("fr-fr")), (k, 1))
    want = ssw.align_text_batch(gpu_fr, lex, torch.from_numpy(gpu_fr.feat_batch(cep, utt_off=fo)).cuda(),
                                fo, [t.split() for t in texts])
    for u in range(k):
        assert aset.status(u) == want.status(u) == 0
        _same_alignment(aset, want, u)
    aset.free()
    want.free()
    lex.free()


@pytest.mark.parametrize("cfg,msg", [({"transform": "htk"}, "htk"), ({"dither": 1}, "dither"),
                                     ({"samprate": 8000.0}, "samprate")])
def test_refusals(gpu_en, cfg, msg):
    with pytest.raises(ssw.SswError, match=msg):
        gpu_en.fe_batch(_raw("goforward.raw"), cfg=cfg)


def test_both_models_load_with_their_feat_params(gpu_en, gpu_fr):
    for g in (gpu_en, gpu_fr):
        c = g.fe_config()
        assert c.from_file == 1 and c.nfilt == 20 and c.remove_noise == 1 and c.transform == 1


def test_kernel_timing(gpu_en):
    gpu_en.set_kernel_timing(True)
    try:
        gpu_en.fe_batch(_raw("goforward.raw"))
        ms = gpu_en.fe_kernel_timing()
    finally:
        gpu_en.set_kernel_timing(False)
    assert len(ms) == 3 and all(t > 0 for t in ms)
