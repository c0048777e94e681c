"""The exact in-wave pass of the two top-N scans (the `while (todo)` loops of
ptm_topn_mfma_kernel and ptm_topn_frames_kernel; what they must do: csrc/ssw_scan_common.inc) at
the smallest shape that reaches every arm of its choice of the carried order.

Three utterances of 1, 63 and 131 frames: utterance starts at frames 0, 1 and 64, a wave boundary
at 64 and 128, a second 64-frame step under SSW_MFMA_STEPS=2, a one-frame utterance, utterances of
odd length (the chain over utterances steps over their last frames).  Runs of identical frames
whose truncated scores tie among the four best sit on all of those places, so the pairs there are
unproven by construction and go through the reference's state machine with the order their
predecessor left.  Expected: the sequential chain kernel (a model loaded with SSW_PTM_EXACT=1),
entry by entry."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_alignment_task, synth_features
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu

LENS = (1, 63, 131)
OFF = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int32)
N = int(OFF[-1])
# utterance starts, wave boundaries, one frame strictly inside a wave, the last frame
TIE_AT = (0, 1, 64, 128, 37, N - 1)
# runs of one tying frame each: [first, last + 1, which of the tying candidates]
RUNS = ((0, 3, 0), (30, 41, 1), (62, 67, 2), (126, 131, 3), (N - 5, N, 0))


def _top4_tie_pairs(orc, means, x):
    """per frame: the (codebook, stream) pairs whose four best truncated densities hold two equal
    ints.  Reference arithmetic in numpy float32, one rounding per operation."""
    n_cb, n_feat, n_den, vl = means.shape
    mean = orc.mean.reshape(means.shape)
    var = orc.var.reshape(means.shape)
    det = orc.det.reshape(n_cb, n_feat, n_den)
    x = np.ascontiguousarray(x, np.float32).reshape(len(x), 1, n_feat, 1, vl)
    d = np.broadcast_to(det, (x.shape[0],) + det.shape).astype(np.float32).copy()
    for j in range(vl):
        diff = x[..., j] - mean[None, ..., j]
        d = d - (diff * diff) * var[None, ..., j]
    iv = np.trunc(np.maximum(d, np.float32(-2147483648.0))).astype(np.int64)
    top = -np.sort(-iv, axis=-1)[..., :4]
    return ((top[..., :-1] == top[..., 1:]).any(axis=-1)).reshape(len(x), -1).sum(axis=1)


def _tie_batch(orc, means):
    """filler frames with runs of tie-making frames on RUNS (the construction of
    test_gpu_ptm.py's tie-heavy batches, cut down to N frames)"""
    cand = (np.round(synth_features(means, 600, 31337) * 8.0) / 8.0).astype(np.float32)
    ties = cand[np.argsort(-_top4_tie_pairs(orc, means, cand), kind="stable")[:4]]
    filler = synth_features(means, 64, 999)
    feats = filler[np.random.default_rng(5).integers(0, len(filler), N)].copy()
    for a, b, k in RUNS:
        feats[a:b] = ties[k]
    return np.ascontiguousarray(feats, np.float32)


def _tied_frames(sc):
    """[n] bool: some (codebook, stream) of the frame shows two equal scores among its four"""
    s = np.sort(sc.reshape(len(sc), -1, sc.shape[-1]), axis=-1)
    return (s[..., :-1] == s[..., 1:]).any(axis=-1).any(axis=-1)


def _pack(cw):
    c = cw.reshape(-1, 4).astype(np.uint32)
    return (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32)


@pytest.fixture(scope="module")
def exact(orc_en, means_en):
    """the batch and what the chain kernel makes of it: rows, codewords, scores; and the same as
    ONE chain over the utterances from a carried-in order"""
    os.environ["SSW_PTM_EXACT"] = "1"
    try:
        gx = ssw.Model(ssw.model_dir("en-us"))
    finally:
        del os.environ["SSW_PTM_EXACT"]
    feats = _tie_batch(orc_en, means_en)
    rows = gx.score_batch(feats, OFF)
    flagged, pairs = gx.last_stats()
    assert flagged == pairs == N * 126                  # the chain kernel, every pair
    cw, sc = gx.last_topn(N)
    tied = _tied_frames(sc)
    assert all(tied[t] for t in TIE_AT), [(t, bool(tied[t])) for t in TIE_AT]
    # carried in: frame 0's own four, worst first -- codewords that tie there are re-scored in the
    # carried order and keep it (eval_topn is a stable insertion), so the tie breaks the other way
    carry_in = _pack(cw[0][..., ::-1])
    assert (carry_in != 0x03020100).any()
    crows, ccarry = gx.score_batch_carry(feats, OFF, carry_in=carry_in, carry_utts=True)
    ccw, csc = gx.last_topn(N)
    assert _tied_frames(csc)[list(TIE_AT)].all()
    yield dict(feats=feats, rows=rows, cw=cw, sc=sc, carry_in=carry_in, crows=crows,
               ccarry=ccarry, ccw=ccw, csc=csc)
    gx.close()


def _same(got, cw, sc, want, wcw, wsc):
    assert np.array_equal(cw, wcw)
    assert np.array_equal(sc, wsc)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("knobs", [{}, {"SSW_MFMA_STEPS": "2"}, {"SSW_SCAN": "fma"},
                                   {"SSW_SCAN_AUDIT": "1"}],
                         ids=["default", "steps2", "fma", "audit"])
def test_scans_agree_with_the_chain_kernel(gpu_en, exact, monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    got = gpu_en.score_batch(exact["feats"], OFF)
    flagged, pairs = gpu_en.last_stats()
    cw, sc = gpu_en.last_topn(N)
    print("knobs %s: %d of %d pairs through the exact pass" % (knobs, flagged, pairs))
    assert pairs == N * 126 and 0 < flagged < pairs
    _same(got, cw, sc, exact["rows"], exact["cw"], exact["sc"])
    if "SSW_SCAN_AUDIT" in knobs:
        audited, differ = gpu_en.scan_audit_stats()
        assert audited > 0 and differ == 0
        assert audited + flagged == pairs               # k = 1: every wave redoes all its frames


def test_chain_over_utterances_from_a_carried_order(gpu_en, exact):
    got, carry = gpu_en.score_batch_carry(exact["feats"], OFF, carry_in=exact["carry_in"],
                                          carry_utts=True)
    flagged, pairs = gpu_en.last_stats()
    cw, sc = gpu_en.last_topn(N)
    assert 0 < flagged < pairs
    _same(got, cw, sc, exact["crows"], exact["ccw"], exact["csc"])
    assert np.array_equal(carry, exact["ccarry"])
    # the carried order and the chain matter on this input
    assert not np.array_equal(exact["ccw"], exact["cw"])


def test_masked_call_on_the_same_frames(gpu_en, orc_en, oracle_mod, exact):
    """compallsen = no through align_batch_active: per frame only the codebooks of the search's
    active senones are scanned, the others' pairs are nobody's input and their orders are
    re-derived when they come back.  Against the oracle's per-frame scorer driven by the restated
    search (tests/test_gpu_active.py)."""
    from tests.test_gpu_active import INT_MAX, second_pass_active
    feats = exact["feats"]
    n_ph = (1, 12, 30)
    senids, tmats, refs = [], [], []
    for u, n in enumerate(n_ph):
        senid, tmat, _ = synth_alignment_task(orc_en.sseq, orc_en.phone_ssid, orc_en.phone_tmat,
                                              orc_en.n_ciphone, n, 700 + u)
        sf, ef = np.zeros(n, np.int32), np.full(n, INT_MAX, np.int32)
        refs.append(second_pass_active(oracle_mod, orc_en, feats[OFF[u]:OFF[u + 1]], senid, tmat,
                                       sf, ef, None))
        senids.append(senid)
        tmats.append(tmat)
    phone_off = np.concatenate([[0], np.cumsum(n_ph)]).astype(np.int32)
    d_feats = gpu_en.to_device(feats)
    d_scr = gpu_en.device_malloc(N * gpu_en.n_sen * 2)
    try:
        st, status = gpu_en.align_batch_active(d_feats, OFF, phone_off, np.concatenate(senids),
                                               np.concatenate(tmats), d_senscr=d_scr)
        flagged, _ = gpu_en.last_stats()
        scr = np.zeros((N, gpu_en.n_sen), np.int16)
        gpu_en._L.ssw_memcpy_d2h(scr.ctypes.data, d_scr, scr.nbytes)
    finally:
        gpu_en.device_free(d_feats)
        gpu_en.device_free(d_scr)
    assert flagged > 0
    assert any(r[0] == 0 for r in refs)
    for u, (rv, rst, rows) in enumerate(refs):
        assert np.array_equal(scr[OFF[u]:OFF[u + 1]], rows), u
        assert (status[u] == 0) == (rv == 0), u
        if rv == 0:
            assert np.array_equal(st[phone_off[u] * 3:phone_off[u + 1] * 3], rst), u


def test_ms_scorer_same_lengths(oracle_mod, orc_fr, means_fr, tmp_path, monkeypatch):
    """the ms scorer keeps no history (ms_exact_step): fr-fr with mixture weights made from its
    sendump, against the oracle's ms scores, on both scans"""
    from tests.test_cabi_host import synth_mixw_from_sendump
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    g = ssw.Model(variances=os.path.join(src, "variances"), **kw)
    o = oracle_mod.Model(vars=os.path.join(src, "variances"), **kw)
    try:
        feats = _tie_batch(orc_fr, means_fr)
        want = o.ms_score_utt(feats)
        for scan in (None, "fma"):
            if scan:
                monkeypatch.setenv("SSW_SCAN", scan)
            got = g.score_batch(feats, OFF, scorer=ssw.SCORER_MS)
            flagged, pairs = g.last_stats()
            print("ms, scan %s: %d of %d pairs through the exact pass" % (scan, flagged, pairs))
            assert 0 < flagged < pairs
            assert np.array_equal(got, want)
    finally:
        g.close()
