"""The host side of a scoring call (score_batch_impl, soundswallower_amd/csrc/ssw_host_score.inc):
what it keeps from call to call on one model -- the cached offsets and their start / skip bits, the
staging slot the carried rows share with them, the stream of the last call, the top-N workspace
that ssw_score_batch_host's pieces write stretches of, the timing events -- against the CPU oracle
on en-us.  Nothing is tolerated: int16 rows, codeword orders and counters are compared for
equality."""
import ctypes

import numpy as np
import pytest
import torch

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_features
from tests import sc_common as S
from tests.test_gpu_ptm import _unprovable_pairs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fresh_en():
    """a model of its own: the calls below speak of what earlier calls left on it"""
    g = ssw.Model(ssw.model_dir("en-us"))
    yield g
    g.close()


def _pack(cw):
    """codewords [n_cb][n_feat][4], best first -> carry rows uint32 [n_cb * n_feat]"""
    c = np.asarray(cw, np.uint32).reshape(-1, 4)
    return (c[:, 0] | (c[:, 1] << 8) | (c[:, 2] << 16) | (c[:, 3] << 24)).astype(np.uint32)


def _oracle_call(o, feats, off, chain, pre=None):
    """One ssw_score_batch_ex call restated frame by frame: (rows, carry_out).  chain: the history
    runs through the utterances (SSW_SCORE_CARRY_UTTS), else every utterance but the first starts
    from the reset history.  pre: frames scored ahead of utterance 0, which continues them -- what
    a carry_in of their last frame's order means (an even count: the ring's parity is kept)."""
    o.ptm_reset()
    base0 = 0
    if pre is not None:
        assert len(pre) % 2 == 0
        for i in range(len(pre)):
            o.ptm_set_frame_idx(i)
            o.ptm_frame_eval(pre[i], i)
        base0 = len(pre)
    out = np.zeros((len(feats), o.n_sen), np.int16)
    last = None
    for u in range(len(off) - 1):
        if u > 0 and not chain:
            o.ptm_reset()
        base = base0 if u == 0 else 0
        for i, t in enumerate(range(int(off[u]), int(off[u + 1]))):
            o.ptm_set_frame_idx(base + i)
            out[t] = o.ptm_frame_eval(feats[t], base + i)
            last = base + i
        o.ptm_set_frame_idx(last + 1)
    return out, _pack(o.ptm_get_topn(last)[0])


def _history_frames(o, means):
    """(12 frames, 4 frames to score ahead of them) on which the history a frame starts from shows
    in its row: frames y, z, x found with the oracle such that x scored after y differs from x
    scored after z (as tests/test_gpu_ptm.py::_ring_features finds its triplets), and from x
    scored first in an utterance.  As utterances of 5, 1 and 6 frames the x at frame 5 starts from
    the reset history, or from y's order with the history carried (y has the odd number 3, the z
    behind it is off the ring); as 4, 4, 4 it follows z; the x at frame 0 follows the y that ends
    the frames ahead."""
    cand = (np.round(synth_features(means, 600, 31337) * 8.0) / 8.0).astype(np.float32)
    bad = _unprovable_pairs(o, means, cand).reshape(len(cand), -1).sum(axis=1)
    for xi in np.argsort(-bad)[:8]:
        first = o.ptm_score_utt(cand[xi:xi + 1])[0].tobytes()
        rows = {}
        for yi in range(60):
            rows.setdefault(o.ptm_score_utt(np.stack([cand[yi], cand[xi]]))[1].tobytes(), yi)
        if len(rows) >= 2:
            after = sorted(rows.items(), key=lambda kv: kv[0] == first)   # y: not as from the reset
            y, z, x = cand[after[0][1]], cand[after[1][1]], cand[xi]
            f = synth_features(means, 5, 999)
            return (np.stack([x, f[0], z, y, z, x, x, y, z, x, f[1], y]).astype(np.float32),
                    np.stack([f[2], f[3], f[4], y]).astype(np.float32))
    raise AssertionError("no history-sensitive frames among the candidates")


def _device_call(g, feats, off, stream=None):
    """ssw_score_batch on device buffers, on `stream` (a torch stream or None = the default one)"""
    d_in = torch.from_numpy(np.ascontiguousarray(feats, np.float32)).cuda()
    d_out = torch.zeros((len(feats), g.n_sen), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    g.score_batch_device(d_in, len(feats), off, d_out,
                         stream=stream.cuda_stream if stream is not None else None)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def test_offsets_cache_and_the_staging_slot_it_shares(fresh_en, orc_en, means_en):
    """One model, utterances of 5, 1 and 6 frames: chain off, chain on, chain off again (the chain
    flag is part of the cache key; odd and one-frame utterances set skip bits), other offsets of
    the same count (4, 4, 4), then the first offsets with a carry_in, twice (the carried rows go
    through the staging slot with the offsets, then -- the offsets cached -- alone), and the chain
    once more.  Rows and carry_out of every call are the oracle's."""
    g, o = fresh_en, orc_en
    feats, pre = _history_frames(o, means_en)
    off_a = np.array([0, 5, 6, 12], np.int32)
    off_b = np.array([0, 4, 8, 12], np.int32)
    _, carry = _oracle_call(o, pre, [0, 4], False)
    calls = [(off_a, False, None), (off_a, True, None), (off_a, False, None), (off_b, False, None),
             (off_a, False, carry), (off_a, False, carry), (off_a, True, None)]
    for k, (off, chain, cin) in enumerate(calls):
        want, want_carry = _oracle_call(o, feats, off, chain, pre if cin is not None else None)
        got, got_carry = g.score_batch_carry(feats, off, carry_in=cin, carry_utts=chain)
        bad = np.flatnonzero((got != want).any(axis=1))
        print("call %d: offsets %s chain %d carry_in %d: %d rows differ %s" % (
            k, off.tolist(), chain, cin is not None, len(bad), bad.tolist()))
        assert np.array_equal(got, want), k
        assert np.array_equal(got_carry, want_carry), k
    # not a vacuous pass: on these frames the chain flag, the offsets and carry_in show in the rows
    plain, _ = _oracle_call(o, feats, off_a, False)
    chained, _ = _oracle_call(o, feats, off_a, True)
    assert not np.array_equal(plain, chained)
    assert not np.array_equal(chained, _oracle_call(o, feats, off_b, False)[0])
    assert not np.array_equal(plain, _oracle_call(o, feats, off_a, False, pre)[0])


def test_a_caller_that_changes_streams(fresh_en, orc_en, means_en):
    """12 frames on one stream, other offsets on a second stream, then on the default stream: the
    uploads of a call are ordered behind the launches of its own stream only"""
    g, o = fresh_en, orc_en
    feats = synth_features(means_en, 12, 7303)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for off, st in (([0, 12], s1), ([0, 3, 12], s2), ([0, 7, 8, 12], None)):
        off = np.array(off, np.int32)
        want, _ = _oracle_call(o, feats, off, False)
        assert np.array_equal(_device_call(g, feats, off, st), want), off.tolist()


def test_host_call_leaves_the_model_whole(orc_en, means_en, monkeypatch):
    """SSW_HOST_PIPE_CAP=4 on utterances of 10 and 3 frames: three pieces and one group, each
    scoring into its own stretch of the top-N workspace.  The rows are the oracle's; the whole-call
    top-N view and the counters are what ssw_score_batch of the same batch leaves; and the model
    scores a larger batch (300 frames: the workspace grows) as the oracle does."""
    o = orc_en
    g = ssw.Model(ssw.model_dir("en-us"))
    try:
        feats = synth_features(means_en, 13, 7304)
        off = np.array([0, 10, 13], np.int32)
        want, _ = _oracle_call(o, feats, off, False)
        monkeypatch.setenv("SSW_HOST_PIPE_CAP", "4")
        cut = g.score_batch(feats, off)
        monkeypatch.delenv("SSW_HOST_PIPE_CAP")
        cw_cut, sc_cut = g.last_topn(13)
        stats_cut = g.last_stats()
        assert np.array_equal(cut, want)
        plain = _device_call(g, feats, off)
        cw_plain, sc_plain = g.last_topn(13)
        stats_plain = g.last_stats()
        print("stats: host call %s, plain call %s" % (stats_cut, stats_plain))
        assert np.array_equal(plain, want)
        assert np.array_equal(cw_cut, cw_plain) and np.array_equal(sc_cut, sc_plain)
        assert stats_cut == stats_plain
        big = synth_features(means_en, 300, 7305)
        big_off = np.array([0, 299, 300], np.int32)
        assert np.array_equal(_device_call(g, big, big_off), _oracle_call(o, big, big_off, False)[0])
    finally:
        g.close()


def _timing(g):
    ms = np.zeros(3, np.float32)
    n = g._L.ssw_get_kernel_timing(g._m, ms.ctypes.data_as(ctypes.c_void_p), 3)
    assert (ms[:max(n, 0)] >= 0).all()
    return n


def test_kernel_timing_shape(fresh_en, means_en, monkeypatch, tmp_path):
    """ssw_get_kernel_timing: scan and senone kernel of an un-pieced PTM call; one number, the whole
    call, for a call scored in pieces; the chain kernel's share as a third for s2_semi"""
    g = fresh_en
    feats = synth_features(means_en, 512, 7306)
    g.set_kernel_timing(True)
    try:
        _device_call(g, feats, [0, 512])
        assert _timing(g) == 2
        monkeypatch.setenv("SSW_SCORE_PIECE", "256")
        _device_call(g, feats, [0, 512])
        monkeypatch.delenv("SSW_SCORE_PIECE")
        assert _timing(g) == 1
        _device_call(g, feats, [0, 512])
        assert _timing(g) == 2
    finally:
        g.set_kernel_timing(False)
    a = ssw.Model(S.model_a_dir(str(tmp_path / "A")))
    try:
        cep = np.load(S.GOLD + "/goforward_mfcc.npy").astype(np.float32)
        f = np.ascontiguousarray(a.feat_batch(cep), np.float32)[:24]
        a.set_kernel_timing(True)
        _device_call(a, f, [0, 24])
        assert _timing(a) == 3
    finally:
        a.close()
