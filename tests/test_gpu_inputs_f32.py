"""float32 audio on the GPU (ssw_fe_batch_f32: K8's spectrum kernel reading float samples) against
the int16 path on the same audio, against the reference library's own cepstra and alignments of
float audio (tests/golden/inputs_f32.npz, written by tests/golden/make_inputs.py from
fe_process_float32 and decoder_process_float32), and with non-finite samples.  Every comparison of
cepstra is tobytes() equality.

Every test here needs the feature: without it float samples are cut to zeros on the host and a
float tensor is read as int16 pairs on the device."""
import json
import os

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from tests import fe_rates_common as R
from tests import inputs_common as I
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

LEGACY = dict(transform="legacy", remove_noise=False, lifter=0, nfilt=40, lowerf=133.33334,
              upperf=6855.4976)


def _same(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
        f, i = bad[0]
        pytest.fail(f"{what}: {len(bad)} values differ, first frame {f} cep {i}: "
                    f"{got[f, i]!r} vs {want[f, i]!r}")


@pytest.fixture(scope="module")
def gold():
    return np.load(I.F32_NPZ)


@pytest.fixture(scope="module")
def lex(gpu_en):
    d = os.path.join(MODEL_ROOT, "en-us")
    return ssw.Lexicon(gpu_en, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))


def _ragged():
    """the lengths around one window and one shift at two rates mixed, an empty utterance and the
    whole recording at each: (int16 arrays, rates)"""
    pcms, rates = [], []
    for k, n in enumerate(I.edge_lengths(16000)):
        for rate, m in ((16000, n), (44100, I.edge_lengths(44100)[k])):
            pcms.append(I.int_pcm(rate)[3000 + k:3000 + k + m].copy())
            rates.append(rate)
    pcms += [np.zeros(0, np.int16), I.int_pcm(44100), I.int_pcm(16000)]
    rates += [44100, 44100, 16000]
    return pcms, rates


@pytest.mark.parametrize("cfg", [None, LEGACY], ids=["model", "legacy"])
def test_exact_scale_equals_the_int16_path(gpu_en, cfg):
    """x / 32768 through ssw_fe_batch_f32 = x through ssw_fe_batch_ex, from host arrays and from
    device tensors"""
    pcms, rates = _ragged()
    f32 = [I.KINDS["exact"](p) for p in pcms]
    want, wfo = gpu_en.fe_batch_rates(pcms, rates, cfg=cfg)
    got, gfo = gpu_en.fe_batch_rates(f32, rates, cfg=cfg)
    assert list(gfo) == list(wfo) and list(np.diff(wfo)) == list(
        ssw.fe_frame_counts_at([len(p) for p in pcms], rates))
    _same(got, want, "host arrays")
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])])
    d16 = torch.from_numpy(np.concatenate(pcms)).cuda()
    d32 = torch.from_numpy(np.concatenate(f32)).cuda()
    assert d32.dtype == torch.float32
    dwant, _ = gpu_en.fe_batch_rates_device(d16, off, rates, cfg=cfg)
    for how, (dgot, dfo) in (("tensor", gpu_en.fe_batch_rates_device(d32, off, rates, cfg=cfg)),
                             ("f32 entry", gpu_en.fe_batch_f32_device(d32, off, rates, cfg=cfg)),
                             ("pointer", gpu_en.fe_batch_rates_device(
                                 d32.data_ptr(), off, rates, cfg=cfg, pcm_format="f32"))):
        assert list(dfo) == list(wfo)
        _same(dgot.cpu().numpy(), want, how)
    _same(dwant.cpu().numpy(), want, "int16 tensor")
    # 16 kHz alone through the helper that takes no rate
    got16, _ = gpu_en.fe_batch(f32[-1], cfg=cfg)
    want16, _ = gpu_en.fe_batch(pcms[-1], cfg=cfg)
    _same(got16, want16, "fe_batch")
    dgot16, _ = gpu_en.fe_batch_device(torch.from_numpy(f32[-1]).cuda(), [0, len(f32[-1])], cfg=cfg)
    _same(dgot16.cpu().numpy(), want16, "fe_batch_device")


@pytest.mark.parametrize("fx", I.FE_FIXTURES, ids=[f[0] for f in I.FE_FIXTURES])
def test_recorded_fixture(gpu_en, gold, fx):
    """Every recorded float fixture, byte for byte.

    tiny_44100 is the case that needs the correctly rounded logarithm (csrc/ssw_fe_log.inc):
    with the device library's log, one ulp from glibc's at 3 of the fixture's 1980 arguments
    (frame 4 filter 19: log(0x1.a36e310f82520p-14) = -0x1.26bb1b8d1e683p+3 against glibc's
    ...682p+3), 2 of its 99 x 13 values were off by one float32 ulp, -1.9873319e-07 against
    -1.9873318e-07 in frame 4: audio this quiet leaves every mel value next to the 1e-4 floor
    and the DCT cancels the nearly equal logs down to 1e-7 (DESIGN K8, Exactness)."""
    name, kind, rate, cfg, n = fx
    pcm = I.f32_pcm(kind, rate, n)
    want = gold["cep/" + name]
    cep, fo = gpu_en.fe_batch_rates(pcm, rate, cfg=cfg)
    assert list(fo) == [0, len(want)]
    _same(cep, want, name)
    d_cep, fo2 = gpu_en.fe_batch_f32_device(torch.from_numpy(pcm).cuda(), [0, len(pcm)], rate, cfg=cfg)
    assert list(fo2) == [0, len(want)]
    _same(d_cep.cpu().numpy(), want, name + " (device)")


def test_recorded_fixtures_as_one_batch(gpu_en, gold):
    """the fixtures of the model's settings, both rates and every kind, in one call"""
    fxs = [f for f in I.FE_FIXTURES if f[3] == {}]
    assert len(fxs) == len(I.KINDS) + 14
    cep, fo = gpu_en.fe_batch_rates([I.f32_pcm(k, r, n) for _, k, r, _, n in fxs],
                                    [f[2] for f in fxs])
    for u, f in enumerate(fxs):
        _same(cep[fo[u]:fo[u + 1]], gold["cep/" + f[0]], f[0])


def _words_of(line):
    return [(w["t"], w["b"], w["d"]) for w in json.loads(line)["w"]]


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
@pytest.mark.parametrize("case", I.ALIGN_CASES, ids=[f"{k}{r}" for k, r in I.ALIGN_CASES])
def test_float_alignment(gpu_en, gold, lex, case, active):
    kind, rate = case
    ref = gold[I.align_key(kind, rate, "no" if active else "yes")].tobytes().decode("utf-8")
    pcm = I.f32_pcm(kind, rate)
    texts = [I.ALIGN_TEXT.split()]
    sr = None if rate == 16000 else rate
    words = I.ALIGN_TEXT.split()
    plan = lex.grammar_plan(ssw.Fsg.create(gpu_en, lex, I.ALIGN_TEXT, 0, len(words),
                                           [(i, i + 1, 1.0, w) for i, w in enumerate(words)]))
    for audio in (pcm, torch.from_numpy(pcm).cuda()):
        aset = ssw.align_audio_batch(gpu_en, lex, audio, [0, len(pcm)], texts, active=active,
                                     samprate=sr)
        assert aset.status(0) == 0
        assert aset.json(0) == ref
        aset.free()
        rs = ssw.recognize_audio_batch(gpu_en, lex, audio, [0, len(pcm)], plan, samprate=sr,
                                       active=active)
        assert rs.status(0) == 0 and rs.hyp(0) == I.ALIGN_TEXT
        segs = [(s[0], round(s[1] / 100, 3), round((s[2] - s[1] + 1) / 100, 3))
                for s in rs.segments(u=0)]
        assert segs == _words_of(ref)
        rs.free()
        r2, al = ssw.recognize_align_audio_batch(gpu_en, lex, audio, [0, len(pcm)], plan,
                                                 samprate=sr, active=active)
        assert al.json(0) == ref
        al.free()
        r2.free()
    plan.free()


def test_float_and_int16_batches_do_not_mix(gpu_en, lex):
    pcm = I.int_pcm(16000)
    with pytest.raises(ssw.SswError, match="all int16 or all float32"):
        gpu_en.fe_batch_rates([pcm, I.KINDS["exact"](pcm)], 16000)
    with pytest.raises(ssw.SswError, match="torch.float64"):
        gpu_en.fe_batch_rates_device(torch.zeros(1000, dtype=torch.float64).cuda(), [0, 1000], 16000)
    with pytest.raises(ssw.SswError, match="torch.float16"):
        ssw.align_audio_batch(gpu_en, lex, torch.zeros(1000, dtype=torch.float16).cuda(), [0, 1000],
                              [["go"]])


def test_non_finite_samples(gpu_en):
    """one NaN and one Inf in the middle of 1 s, remove_noise off: the same bytes twice, and every
    frame whose window and prior sample hold neither is the clean run's"""
    cfg = {"remove_noise": False}
    clean = I.f32_pcm("frac", 16000, 16000)
    dirty = clean.copy()
    bad = (8000, 8300)
    dirty[bad[0]], dirty[bad[1]] = np.float32("nan"), np.float32("inf")
    want, fo = gpu_en.fe_batch_rates(clean, 16000, cfg=cfg)
    a, fa = gpu_en.fe_batch_rates(dirty, 16000, cfg=cfg)
    b, _ = gpu_en.fe_batch_rates(dirty, 16000, cfg=cfg)
    assert list(fa) == list(fo) and a.tobytes() == b.tobytes()
    shift, size = R.framing(16000)
    touched = np.array([any(shift * f - 1 <= s < shift * f + size for s in bad)
                        for f in range(len(want))])
    assert 3 <= touched.sum() <= 8
    _same(a[~touched], want[~touched], "frames without a non-finite sample")
    assert not np.isfinite(a[touched]).all()
    # and in a batch the neighbours are untouched
    c, fc = gpu_en.fe_batch_rates([clean, dirty, clean], 16000, cfg=cfg)
    _same(c[fc[0]:fc[1]], want, "before")
    _same(c[fc[2]:fc[3]], want, "after")
    assert c[fc[1]:fc[2]].tobytes() == a.tobytes()
