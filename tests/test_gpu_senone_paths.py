"""GPU parity of the senone kernels that share the steps of csrc/ssw_senone_common.inc, on the
paths no other test pins, bit for bit against the CPU oracle.

The ms scorer's `scr /= aw` (src/ms_senone.c:351-354) sits in ms_senone_kernel,
senone_active2_kernel<true> and senone_listed_kernel<true> through one ms_finish / ms_slot_score:
fr-fr with mixture weights synthesised from the sendump, loaded on both sides with aw = 3 (odd: a
real truncating division, not a shift).  The PTM slot score is one function for ptm_frame_kernel,
senone_active2_kernel<false> and senone_listed_kernel<false>; the packed ms kernel's marked frames
go through the same ms_quad_scores as ms_senone_kernel."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_alignment_task, synth_features
from tests.conftest import MODEL_ROOT
from tests.test_cabi_host import synth_mixw_from_sendump
from tests.test_gpu_active import INT_MAX, _windows, second_pass_active

pytestmark = pytest.mark.gpu


def _ms_models(oracle_mod, orc_fr, tmp, config):
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw, config=config)
    return (ssw.Model(variances=os.path.join(src, "variances"), **kw),
            oracle_mod.Model(vars=os.path.join(src, "variances"), **kw))


@pytest.fixture(scope="module")
def aw3(oracle_mod, orc_fr, tmp_path_factory):
    return _ms_models(oracle_mod, orc_fr, tmp_path_factory.mktemp("aw3"), {"aw": 3})


@pytest.fixture(scope="module")
def aw1(oracle_mod, orc_fr, tmp_path_factory):
    return _ms_models(oracle_mod, orc_fr, tmp_path_factory.mktemp("aw1"), None)


def _active_batch_against_the_restated_search(oracle_mod, g, o, means, cases, ms, seed0):
    """tests/test_gpu_active.py's comparison: one align_batch_active call with full [n_sen] rows
    against second_pass_active around the oracle's frame_eval, every row and every state.
    Returns the utterances' features, their oracle rows and the GPU's."""
    rng = np.random.default_rng(23)
    feats, senids, tmats, sfs, efs, refs = [], [], [], [], [], []
    for k, (n_ph, n_fr, windowed) in enumerate(cases):
        f = synth_features(means, n_fr, seed0 + k)
        senid, tmat, _ = synth_alignment_task(o.sseq, o.phone_ssid, o.phone_tmat, o.n_ciphone,
                                              n_ph, 900 + k)
        sf, ef = _windows(rng, n_ph, n_fr) if windowed else (np.zeros(n_ph, np.int32),
                                                             np.full(n_ph, INT_MAX, np.int32))
        refs.append(second_pass_active(oracle_mod, o, f, senid, tmat, sf, ef, None, ms=ms))
        feats.append(f); senids.append(senid); tmats.append(tmat); sfs.append(sf); efs.append(ef)
    frame_off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.int32)
    phone_off = np.concatenate([[0], np.cumsum([len(s) for s in senids])]).astype(np.int32)
    allf = np.concatenate(feats)
    d_feats = g.to_device(allf)
    d_scr = g.device_malloc(len(allf) * g.n_sen * 2)
    try:
        kw = dict(scorer=ssw.SCORER_MS) if ms else {}
        st, status = g.align_batch_active(d_feats, frame_off, phone_off, np.concatenate(senids),
                                          np.concatenate(tmats), np.concatenate(sfs),
                                          np.concatenate(efs), d_senscr=d_scr, **kw)
        scr = np.zeros((len(allf), g.n_sen), np.int16)
        g._L.ssw_memcpy_d2h(scr.ctypes.data, d_scr, scr.nbytes)
    finally:
        g.device_free(d_feats)
        g.device_free(d_scr)
    assert any(r[0] == 0 for r in refs)
    for u, (rv, rst, rows) in enumerate(refs):
        a, b = frame_off[u], frame_off[u + 1]
        bad = np.argwhere(scr[a:b] != rows)
        assert len(bad) == 0, ("scores", u, len(bad), bad[:6].tolist(),
                               [(int(scr[a + i, j]), int(rows[i, j])) for i, j in bad[:6]])
        assert (status[u] == 0) == (rv == 0), u
        if rv == 0:
            assert np.array_equal(st[phone_off[u] * 3:phone_off[u + 1] * 3], rst), ("states", u)
    return feats, [r[2] for r in refs], [scr[frame_off[u]:frame_off[u + 1]] for u in range(len(cases))]


@pytest.mark.parametrize("generic", [False, True])
def test_ms_senone_kernel_divides_by_aw(aw3, means_fr, monkeypatch, generic):
    """aw != 1 always takes ms_senone_kernel; with SSW_SEN_GENERIC=1 its instance with the stream
    count as a run-time value."""
    if generic:
        monkeypatch.setenv("SSW_SEN_GENERIC", "1")
    g, o = aw3
    lens = [33, 1, 70]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    feats = np.concatenate([synth_features(means_fr, n, 12345 + i) for i, n in enumerate(lens)])
    got = g.score_batch(feats, off, scorer=ssw.SCORER_MS)
    ref = o.ms_score_utt(feats)
    assert np.array_equal(got, ref)


def test_active2_kernel_ms_divides_by_aw(aw3, oracle_mod, means_fr):
    """senone_active2_kernel<true>: full [n_sen] rows and states of a batch with active lists."""
    g, o = aw3
    _active_batch_against_the_restated_search(oracle_mod, g, o, means_fr,
                                              [(6, 40, False), (9, 70, True)], True, 5100)


def test_listed_kernel_ms_divides_by_aw(aw3, oracle_mod):
    """senone_listed_kernel<true>: the first pass in the default configuration on the French
    recording with one short text; the segmentation and every frame's listed entries."""
    import torch
    from oracle import fsg_oracle as F
    from tests.test_gpu_first_pass_active import _cep_batch, oracle_default_first_pass
    O = oracle_mod
    g, o = aw3
    src = os.path.join(MODEL_ROOT, "fr-fr")
    olex = F.Lexicon(o, os.path.join(src, "dict.txt"), os.path.join(src, "noisedict.txt"))
    lex = ssw.Lexicon(g, os.path.join(src, "dict.txt"), os.path.join(src, "noisedict.txt"))
    text = ["avance"]
    feats, off, n = _cep_batch(g, "goforward_fr_mfcc.npy", 1)
    d_feats = torch.from_numpy(feats).cuda()
    d_rows = torch.zeros((len(feats), g.n_sen), dtype=torch.int16, device="cuda")
    segs, rounds = lex.first_pass_active(d_feats, off, [text], scorer=ssw.SCORER_MS, d_senscr=d_rows)
    torch.cuda.synchronize()
    rows = d_rows.cpu().numpy()
    listed = []
    real = O.flags2list                          # spy: which entries each frame lists

    def spy(vec, n_sen):
        lst = real(vec, n_sen)
        listed.append(np.cumsum(np.asarray(lst, np.int64)))
        return lst
    O.flags2list = spy
    try:
        w, wrows, _ = oracle_default_first_pass(O, F, o, olex, text, feats[:n], ms=True)
    finally:
        O.flags2list = real
    assert w is not None and len(listed) == n
    assert [(x, s, s + d - 1, sc) for (x, s, d, sc) in segs[0]] == w
    for f, ids in enumerate(listed):
        assert np.array_equal(rows[f, ids], wrows[f, ids]), f


def test_ms_vtable_with_an_active_list_divides_by_aw(aw3, oracle_mod, means_fr):
    """MsMgau.frame_eval(compallsen=False): ms_senone_kernel's un-normalised mode, the listed
    senones normalised by the best of them."""
    g, o = aw3
    mg = ssw.MsMgau(g)
    rng = np.random.default_rng(9)
    feats = synth_features(means_fr, 4, 2)
    for t, dens in enumerate((0.01, 0.2, 1.0, 0.05)):
        vec = np.zeros((o.n_sen + 31) // 32, np.uint32)
        for s in np.flatnonzero(rng.random(o.n_sen) < dens):
            vec[s // 32] |= np.uint32(1 << (s % 32))
        lst = oracle_mod.flags2list(vec, o.n_sen)
        got = mg.frame_eval(feats[t], t, compallsen=False, senone_active=lst)
        ref = o.ms_frame_eval(feats[t], t, compallsen=False, senone_active=lst)
        assert np.array_equal(got, ref), t
    mg.free()


def test_ptm_twins_give_the_oracles_rows(gpu_en, orc_en, oracle_mod, means_en):
    """One 30-frame utterance and a 6-phone alignment, default settings: the frames' active lists
    through ptm_frame_kernel (the vtable call) and through senone_active2_kernel<false> (the batch
    call, full rows) -- both the oracle's ptm_frame_eval rows, so three equal rows per frame."""
    O = oracle_mod
    lists = []
    real = O.flags2list

    def spy(vec, n_sen):
        lst = real(vec, n_sen)
        lists.append(np.array(lst, copy=True))
        return lst
    O.flags2list = spy
    try:
        feats, want, got = _active_batch_against_the_restated_search(
            O, gpu_en, orc_en, means_en, [(6, 30, False)], False, 4000)
    finally:
        O.flags2list = real
    feats, want, got = feats[0], want[0], got[0]
    assert len(lists) == len(feats) == 30
    mg = ssw.PtmMgau(gpu_en)
    try:
        for t in range(len(feats)):
            row = mg.frame_eval(feats[t], t, compallsen=False, senone_active=lists[t])
            assert np.array_equal(row, want[t]), t
            assert np.array_equal(row, got[t]), t
            mg.frame_idx = t + 1
    finally:
        mg.free()


def test_packed_ms_kernel_marked_frames_at_its_threshold(aw1, means_fr, monkeypatch):
    """2,048 + 3 frames: the smallest batch the packed persistent kernel takes, with a ragged last
    unit.  Four frames scaled by 100 .. 3000 and an all-zero one are marked and redone by
    ms_exact_frame (the shared ms_quad_scores); every frame equals ms_senone_kernel's
    (SSW_MS_SENONE=old), the special frames and their neighbours equal the oracle's."""
    g, o = aw1
    n = 2048 + 3
    feats = np.ascontiguousarray(synth_features(means_fr, n, 321), np.float32)
    special = {100: 100.0, 777: 300.0, 1500: 1000.0, n - 1: 3000.0, 7: 0.0}
    for t, s in special.items():
        feats[t] *= np.float32(s)
    got = g.score_batch(feats, scorer=ssw.SCORER_MS)
    monkeypatch.setenv("SSW_MS_SENONE", "old")
    old = g.score_batch(feats, scorer=ssw.SCORER_MS)
    monkeypatch.delenv("SSW_MS_SENONE")
    bad = np.nonzero((got != old).any(axis=1))[0]
    assert len(bad) == 0, bad[:10]
    for t in sorted(special):
        a, b = max(t - 1, 0), min(t + 2, n)
        assert np.array_equal(got[a:b], o.ms_score_utt(feats[a:b])), (t, special[t])
