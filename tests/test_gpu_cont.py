"""The ms scorer on continuous-density models on the GPU (csrc/ssw_k11_cont.inc): the models C3,
C3-ties and C1 (tests/cont_common.py) against the reference's recorded rows and results
(tests/golden/cont_results.json) and, for the shapes the reference cannot load, against the numpy
restatement that test_cont_fixture.py holds to those records."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from soundswallower_amd.synth import synth_features
from tests import cont_common as CC
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

MS = ssw.SCORER_MS
CUT = (1, 2, 3, 7, 64)
TILE = 4  # frames per lane of cont_score_kernel (CONT_FR)
# (n_sen, stream lengths, densities, topn): every value the kernel takes another path at --
# senones: 2, a wave - 1, a wave + 1, two waves + 2, more than one workgroup; 1, 2, 4, 8 streams of
# 1, 13, 39, 64 dimensions; 1, 2, topn, topn + 1 and 64 densities; topn 1 .. 8 and all (0)
SHAPES = [
    (2, (1,), 1, 1),
    (63, (13, 13), 2, 1),
    (65, (39,), 4, 4),
    (65, (39,), 5, 4),
    (130, (64, 1, 13, 2), 64, 8),
    (130, (3,) * 8, 9, 8),
    (65, (5,), 12, 2),
    (65, (5,), 12, 3),
    (65, (5,), 12, 5),
    (65, (5,), 12, 6),
    (63, (5,), 12, 7),
    (130, (2,), 64, 0),
    (300, (13,), 3, 2),
]


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("cont_gpu"))
    d = {n: b(os.path.join(tmp, n)) for n, b in CC.BUILDERS.items()}
    d["tmp"] = tmp
    return d


@pytest.fixture(scope="module")
def fx():
    return CC.results()


@pytest.fixture(scope="module")
def feats():
    return CC.features()


@pytest.fixture(scope="module")
def model_c3(dirs):
    m = ssw.Model(**CC.model_paths(dirs["C3"]))
    assert m.continuous and m.scorer() == MS
    return m


def _check_rows(rows, rec):
    got = CC.row_crcs(rows)
    bad = [t for t in range(len(got)) if got[t] != rec["row_crc"][t]]
    assert not bad, "frames %s ... differ from the reference's" % bad[:8]
    for t, row in rec["rows"].items():
        assert np.array_equal(rows[int(t)], np.array(row, np.int16)), t


def _device_rows(m, feats, off):
    d_in = m.to_device(feats)
    out = np.zeros((len(feats), m.n_sen), np.int16)
    d_out = m.device_malloc(out.nbytes)
    try:
        m.score_batch_device(d_in, len(feats), off, d_out)
        assert m._L.ssw_memcpy_d2h(out.ctypes.data, d_out, out.nbytes) == 0
    finally:
        m.device_free(d_in)
        m.device_free(d_out)
    return out


@pytest.mark.parametrize("case", sorted(CC.CASES))
def test_recorded_case(dirs, fx, feats, case):
    model, topn, aw, mixwfloor, scale = CC.CASES[case]
    m = ssw.Model(**CC.model_paths(dirs[model]), config=dict(topn=topn, aw=aw, mixwfloor=mixwfloor))
    assert m.continuous
    x = feats * np.float32(fx["scale"] if scale != 1 else 1)
    _check_rows(_device_rows(m, x, [0, len(x)]), fx["scoring"][case])


def test_host_entry_point_equals_the_device_one(model_c3, feats, fx, monkeypatch):
    """ssw_score_batch_host on 300 frames cut into utterances, one of them longer than the
    pipeline's cap: its pieces are scored as sub-batches of their own"""
    x = np.concatenate([feats, feats[:22]])
    off = np.array([0, 1, 3, 6, 13, 77, 300], np.int32)
    want = _device_rows(model_c3, x, off)
    _check_rows(want[:278], fx["scoring"]["C3"])
    assert np.array_equal(want[278:], want[:22])
    assert np.array_equal(model_c3.score_batch(x, utt_off=off), want)
    monkeypatch.setenv("SSW_HOST_PIPE_CAP", "10")
    assert np.array_equal(model_c3.score_batch(x, utt_off=off), want)
    got, carry = model_c3.score_batch_carry(x[:9], utt_off=[0, 4, 9], carry_utts=True)
    assert np.array_equal(got, want[:9]) and (carry == 0x03020100).all()


@pytest.mark.parametrize("n_sen,veclen,n_density,topn", SHAPES)
def test_synthetic_shape_equals_the_restatement(dirs, n_sen, veclen, n_density, topn):
    name = "syn_%d_%s_%d_%d" % (n_sen, "x".join(map(str, veclen)), n_density, topn)
    d = CC.synthetic_dir(os.path.join(dirs["tmp"], name), n_sen, veclen, n_density, 1000 + n_sen)
    m = ssw.Model(**CC.model_paths(d, mdef=False), config=dict(topn=topn))
    assert m.continuous and m.n_sen == n_sen and m.topn == (topn or n_density)
    x = CC.synthetic_features(sum(CUT), sum(veclen), 77 + n_density)
    want = CC.restated_from_model(m).score(x)
    assert want.any()
    off = np.concatenate([[0], np.cumsum(CUT)]).astype(np.int32)
    assert np.array_equal(m.score_batch(x, utt_off=off), want)
    # a call of 1, 2, a tile - 1, a tile, a tile + 1 frames
    for n in (1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
        assert np.array_equal(_device_rows(m, x[5:5 + n], [0, n]), want[5:5 + n]), n


def test_aw_and_a_nan_row_on_a_synthetic_model(dirs):
    d = CC.synthetic_dir(os.path.join(dirs["tmp"], "syn_aw"), 65, (7, 3), 6, 4242)
    m = ssw.Model(**CC.model_paths(d, mdef=False), config=dict(topn=2, aw=3))
    x = CC.synthetic_features(9, 10, 5)
    want = CC.restated_from_model(m, aw=3).score(x)
    assert np.array_equal(m.score_batch(x), want)
    # a NaN and an infinite feature: the call returns, the other rows are the restatement's, the
    # rows themselves are the same on every call
    bad = x.copy()
    bad[3, 2] = np.nan
    bad[4, 9] = np.inf
    got = m.score_batch(bad)
    keep = [0, 1, 2, 5, 6, 7, 8]
    assert np.array_equal(got[keep], want[keep])
    assert np.array_equal(m.score_batch(bad), got)


def _delta_list(sens):
    out, last = [], 0
    for s in sens:
        d = s - last
        while d > 255:
            out.append(255)
            d -= 255
        out.append(d)
        last = s
    return np.array(out, np.uint8)


def test_ms_mgau_drop_in(model_c3, feats, fx):
    g = ssw.MsMgau(model_c3)
    assert g.name == "ms"
    want = model_c3.score_batch(feats[:12])
    for t in range(12):
        g.frame_idx = t
        assert np.array_equal(g.frame_eval(feats[t], t), want[t]), t
    # compallsen = no: the listed senones (bridge entries included), normalised by the best of
    # them (src/ms_mgau.c:342-364); the restatement gives the raw scores
    lst = _delta_list([0, 5, 700, 701, 5125])
    listed = np.cumsum(lst.astype(np.int64))
    raw = CC.restated_from_model(model_c3).score(feats[:3], raw=True).astype(np.int64)
    for t in range(3):
        row = g.frame_eval(feats[t], t, compallsen=False, senone_active=lst)
        assert np.array_equal(row[listed], raw[t][listed] - raw[t][listed].min()), t
    g.prescore(feats)
    _check_rows(np.stack([g.frame_eval(feats[t], t) for t in range(len(feats))]),
                fx["scoring"]["C3"])
    g.free()
    with pytest.raises(ssw.SswError, match="continuous"):
        ssw.PtmMgau(model_c3)


# ------------------------------------------------------------------------------------------
# end to end on C3
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lex_c3(model_c3, dirs):
    return ssw.Lexicon(model_c3, os.path.join(dirs["C3"], "dict.txt"),
                       os.path.join(dirs["C3"], "noisedict.txt"))


def _pcm():
    return np.fromfile(os.path.join(CC.GOLD, "goforward.raw"), dtype="<i2")


@pytest.mark.parametrize("grammar", ["goforward", "loop", "nulls"])
def test_recognize_audio_batch(model_c3, lex_c3, fx, grammar):
    pcm = _pcm()
    fsg = ssw.Fsg.read(model_c3, lex_c3, os.path.join(CC.GOLD, "fsg", grammar + ".fsg"))
    plan = lex_c3.grammar_plan(fsg)
    r = ssw.recognize_audio_batch(model_c3, lex_c3, pcm, [0, len(pcm)], plan)
    assert r.status(0) == 0, r.message(0)
    rec = fx["rec"][grammar]
    assert {"hyp": r.hyp(0), "score": r.score(0), "segments": [list(s) for s in r.segments(0)],
            "json": r.json(0)} \
        == {"hyp": rec["hyp"], "score": rec["score"], "segments": [s[:5] for s in rec["segments"]],
            "json": rec["json"]}
    r.free()
    with pytest.raises(ssw.SswError, match="continuous"):
        ssw.recognize_audio_batch(model_c3, lex_c3, pcm, [0, len(pcm)], plan, active=True)


def test_align_audio_batch(model_c3, lex_c3, fx):
    pcm = _pcm()
    words = ["go forward ten meters".split()]
    a = ssw.align_audio_batch(model_c3, lex_c3, pcm, [0, len(pcm)], words)
    assert a.status(0) == 0, a.message(0)
    assert a.json(0).rstrip("\n") == fx["align"]["json"].rstrip("\n")
    a.free()
    with pytest.raises(ssw.SswError, match="continuous"):
        ssw.align_audio_batch(model_c3, lex_c3, pcm, [0, len(pcm)], words, active=True)


def test_first_pass_and_forced_alignment_read_whole_rows(model_c3, lex_c3, feats):
    words = ["go forward ten meters".split()]
    d = model_c3.to_device(feats)
    d_scr = model_c3.to_device(model_c3.score_batch(feats))
    try:
        seg = lex_c3.first_pass(d_scr, [0, len(feats)], words)
        assert seg[0] is not None
        a = ssw.align_text_batch(model_c3, lex_c3, d, [0, len(feats)], words)
        assert a.status(0) == 0, a.message(0)
        a.free()
        with pytest.raises(ssw.SswError, match="ssw_first_pass_batch_active.*continuous"):
            lex_c3.first_pass_active(d, [0, len(feats)], words)
        with pytest.raises(ssw.SswError, match="ssw_align_text_batch_active.*continuous"):
            ssw.align_text_batch_active(model_c3, lex_c3, d, [0, len(feats)], words)
    finally:
        model_c3.device_free(d)
        model_c3.device_free(d_scr)


def test_refusals(model_c3, feats, monkeypatch):
    L = model_c3._L
    d_in = model_c3.to_device(feats[:8])

    def refused(rv, who):
        assert rv == -1 and who in _lib.last_error() and "continuous" in _lib.last_error(), \
            _lib.last_error()

    try:
        with pytest.raises(ssw.SswError, match="ssw_compact_plan_create.*continuous"):
            ssw.CompactPlan(model_c3, [0, 8], [0, 2], np.zeros((2, 3), np.uint16))
        refused(L.ssw_score_batch_compact(model_c3._m, MS, d_in, None, None, None, 0),
                "ssw_score_batch_compact")
        refused(L.ssw_align_batch_active_ex(model_c3._m, MS, d_in, 1, None, None, None, None, None,
                                            None, None, None, None, None, None),
                "ssw_align_batch_active")
        refused(L.ssw_score_batch_topn(model_c3._m, 1, None, None), "ssw_score_batch_topn")
        refused(L.ssw_debug_scan_keys(model_c3._m, d_in, 8, 0, None), "ssw_debug_scan_keys")
        refused(L.ssw_debug_scan_top5(model_c3._m, None, 8, None, None), "ssw_debug_scan_top5")
        with pytest.raises(ssw.SswError, match="SSW_SCORER_MS"):
            model_c3.score_batch(feats[:2], scorer=ssw.SCORER_PTM)
        with pytest.raises(ssw.SswError, match="SSW_SCORER_MS"):
            model_c3.score_batch(feats[:2], scorer=ssw.SCORER_S2_SEMI)
        monkeypatch.setenv("SSW_SCAN", "fma")
        with pytest.raises(ssw.SswError, match="SSW_SCAN.*continuous"):
            model_c3.score_batch(feats[:2])
    finally:
        model_c3.device_free(d_in)


def test_other_models_score_the_same_around_a_continuous_batch(model_c3, gpu_en, gpu_fr, means_en,
                                                               means_fr, feats, fx, orc_fr,
                                                               tmp_path):
    """the workspaces are the models' own: an en-us PTM batch and a fr-fr ms batch before and
    after a continuous batch in the same process"""
    from tests.test_cabi_host import synth_mixw_from_sendump
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    fr = ssw.Model(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
                   variances=os.path.join(src, "variances"),
                   tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    assert not fr.continuous and not gpu_en.continuous
    x_en, x_fr = synth_features(means_en, 70, 31), synth_features(means_fr, 70, 32)
    en0 = gpu_en.score_batch(x_en, [0, 33, 70])
    fr0 = fr.score_batch(x_fr, [0, 33, 70], scorer=MS)
    _check_rows(model_c3.score_batch(feats), fx["scoring"]["C3"])
    assert np.array_equal(gpu_en.score_batch(x_en, [0, 33, 70]), en0)
    assert np.array_equal(fr.score_batch(x_fr, [0, 33, 70], scorer=MS), fr0)
    _check_rows(model_c3.score_batch(feats), fx["scoring"]["C3"])
