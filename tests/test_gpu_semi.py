"""The s2_semi scorer on the GPU (csrc/ssw_k10_semi.inc): single-codebook models A, A-ties and B
(tests/sc_common.py) against the reference's recorded rows (tests/golden/sc_results.json) and,
where the reference recorded nothing (cut batches, carried history, a NaN row), against the numpy
restatement that test_sc_fixture.py holds to those records."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd import _lib
from tests import sc_common as S

pytestmark = pytest.mark.gpu

CUT = (1, 2, 3, 7, 64, 201)  # 278 frames: what the reference makes of goforward.raw
SEMI = ssw.SCORER_S2_SEMI


@pytest.fixture(scope="module")
def dirs(tmp_path_factory):
    _lib.build()
    tmp = str(tmp_path_factory.mktemp("sc_gpu"))
    return {"A": S.model_a_dir(os.path.join(tmp, "A")),
            "A-ties": S.model_a_ties_dir(os.path.join(tmp, "A-ties")),
            "B": S.model_b_dir(os.path.join(tmp, "B")), "tmp": tmp}


@pytest.fixture(scope="module")
def model_a(dirs):
    m = ssw.Model(dirs["A"])
    assert m.scorer() == SEMI
    return m


@pytest.fixture(scope="module")
def feats_a(model_a):
    """the 278 goforward frames through ssw_feat_batch: the rows the reference scored"""
    cep = np.load(os.path.join(S.GOLD, "goforward_mfcc.npy")).astype(np.float32)
    f = np.ascontiguousarray(model_a.feat_batch(cep), np.float32)
    assert np.array_equal(f, np.load(S.FEAT_A)), "ssw_feat_batch differs from the reference's rows"
    return f


@pytest.fixture(scope="module")
def fx():
    return S.results()


@pytest.fixture(scope="module")
def restated_a(model_a, feats_a):
    """the restatement over the cut batch, computed once: rows with a reset at every boundary,
    and rows, slot codewords after every utterance, walking the two-slot ring without one"""
    off = np.concatenate([[0], np.cumsum(CUT)]).astype(np.int32)
    r = S.restated_from_model(model_a)
    reset = []
    for u in range(len(CUT)):
        r.reset()
        reset.append(r.utterance(feats_a[off[u]:off[u + 1]]))
    r.reset()
    ring, slots = [], []
    for u in range(len(CUT)):
        ring.append(r.utterance(feats_a[off[u]:off[u + 1]]))
        slots.append((r.slot_codewords(0), r.slot_codewords(1)))
    return off, np.concatenate(reset), np.concatenate(ring), slots


def _pack(cws):
    return np.array([sum(int(c) << (8 * k) for k, c in enumerate(row)) for row in cws], np.uint32)


def _check_rows(rows, rec):
    got = S.row_crcs(rows)
    bad = [t for t in range(len(got)) if got[t] != rec["row_crc"][t]]
    assert not bad, "frames %s ... differ from the reference's" % bad[:8]
    for t, row in rec["rows"].items():
        assert np.array_equal(rows[int(t)], np.array(row, np.int16)), t


def test_model_a_whole_utterance(model_a, feats_a, fx):
    _check_rows(model_a.score_batch(feats_a), fx["scoring"]["A"])
    # the same through the device entry point, the scorer named
    d_in = model_a.to_device(feats_a)
    out = np.zeros((len(feats_a), model_a.n_sen), np.int16)
    d_out = model_a.device_malloc(out.nbytes)
    try:
        model_a.score_batch_device(d_in, len(feats_a), [0, len(feats_a)], d_out, scorer=SEMI)
        assert model_a._L.ssw_memcpy_d2h(out.ctypes.data, d_out, out.nbytes) == 0
    finally:
        model_a.device_free(d_in)
        model_a.device_free(d_out)
    _check_rows(out, fx["scoring"]["A"])


def test_model_a_cut_batch_resets_at_every_boundary(model_a, feats_a, restated_a):
    off, reset, _, _ = restated_a
    got = model_a.score_batch(feats_a, utt_off=off)
    assert np.array_equal(got, reset)
    got2, _ = model_a.score_batch_carry(feats_a, utt_off=off)
    assert np.array_equal(got2, reset)


def test_model_a_cut_batch_carries_the_two_slot_ring(model_a, feats_a, restated_a):
    off, _, ring, slots = restated_a
    got, after_last = model_a.score_batch_carry(feats_a, utt_off=off, carry_utts=True)
    assert np.array_equal(got, ring)
    # default carry_out: the order after the batch's last frame (frame 200 of the last
    # utterance: slot 0); with rewind: slot 1
    assert np.array_equal(after_last, _pack(slots[-1][(CUT[-1] - 1) % 2]))
    _, slot1 = model_a.score_batch_carry(feats_a, utt_off=off, carry_utts=True, rewind=True)
    assert np.array_equal(slot1, _pack(slots[-1][1]))
    # the one-frame utterance leaves slot 1 as it found it: the reset order
    _, s1 = model_a.score_batch_carry(feats_a[:1], utt_off=[0, 1], carry_utts=True, rewind=True)
    assert np.array_equal(s1, np.full(3, 0x03020100, np.uint32))
    assert slots[0][1] == [[0, 1, 2, 3]] * 3
    # a call that continues from carry_out: the batch in two calls, cut at an utterance boundary
    k = int(off[4])                                   # 13 frames: utterances of 1, 2, 3, 7
    first, c1 = model_a.score_batch_carry(feats_a[:k], utt_off=off[:5], carry_utts=True, rewind=True)
    rest, _ = model_a.score_batch_carry(feats_a[k:], utt_off=off[4:] - k, carry_in=c1, carry_utts=True)
    assert np.array_equal(np.concatenate([first, rest]), ring)


def test_model_a_ties(dirs, feats_a, fx):
    """equal densities: equal truncated scores at the list's boundary, where the accept rule and
    the order the history hands on decide"""
    m = ssw.Model(dirs["A-ties"])
    _check_rows(m.score_batch(feats_a), fx["scoring"]["A-ties"])


@pytest.mark.parametrize("topn,ds", S.SETTINGS)
def test_topn_and_ds(dirs, feats_a, fx, topn, ds):
    m = ssw.Model(dirs["A"], config={"topn": topn, "ds": ds})
    rec = fx["scoring"]["A_topn%d_ds%d" % (topn, ds)]
    _check_rows(m.score_batch(feats_a), rec)
    if ds > 1:
        # ssw_score_batch_host cuts the utterance into pieces of 10 frames, which ds = 3 does not
        # divide: a piece keeps its utterance's frame numbers and is handed the history
        old = os.environ.get("SSW_HOST_PIPE_CAP")
        os.environ["SSW_HOST_PIPE_CAP"] = "10"
        try:
            _check_rows(m.score_batch(feats_a), rec)
        finally:
            if old is None:
                del os.environ["SSW_HOST_PIPE_CAP"]
            else:
                os.environ["SSW_HOST_PIPE_CAP"] = old


def test_model_b(dirs, fx):
    """streams of 12, 24, 3 and 12 dimensions, 256 densities: 2 utterances of 32 frames with the
    history carried are the reference's 64 frames (frame 32 starts from slot 1, frame 31's)"""
    m = ssw.Model(dirs["B"])
    assert m.scorer() == SEMI and m.veclen == list(S.B_VECLEN)
    feats = S.model_b_features(S.model_b_tables()[0])
    got, _ = m.score_batch_carry(feats, utt_off=[0, 32, 64], carry_utts=True)
    _check_rows(got, fx["scoring"]["B"])
    _check_rows(m.score_batch(feats), fx["scoring"]["B"])
    # and with a reset between them: the restatement
    r = S.restated_from_model(m)
    want = np.concatenate([r.utterance(feats[:32]), (r.reset(), r.utterance(feats[32:]))[1]])
    assert np.array_equal(m.score_batch(feats, utt_off=[0, 32, 64]), want)


def test_clustered_sendump_scores_as_its_expansion(dirs, feats_a):
    u = S.lcg_uniform(99, 3 * 128 * 5126)
    codes = np.floor(u * 16).astype(np.uint8).reshape(3, 128, 5126)
    codebook = np.array([0, 3, 7, 12, 18, 25, 33, 42, 52, 63, 75, 88, 102, 117, 133, 150], np.uint8)
    d4 = S.model_a_dir(os.path.join(dirs["tmp"], "A4"))
    S.write_sendump4(os.path.join(d4, "sendump"), codebook, codes)
    d8 = S.model_a_dir(os.path.join(dirs["tmp"], "A8"))
    S.write_sendump8(os.path.join(d8, "sendump"), codebook[codes])
    a, b = ssw.Model(d4).score_batch(feats_a[:40]), ssw.Model(d8).score_batch(feats_a[:40])
    assert np.array_equal(a, b) and a.any()


def test_refusals(model_a, feats_a, gpu_en):
    d_in = model_a.to_device(feats_a[:8])
    L = model_a._L
    try:
        with pytest.raises(ssw.SswError, match="s2_semi"):
            ssw.CompactPlan(model_a, [0, 8], [0, 2], np.zeros((2, 3), np.uint16))
        rv = L.ssw_score_batch_compact(model_a._m, SEMI, d_in, None, None, None, 0)
        assert rv == -1 and "ssw_score_batch_compact" in _lib.last_error() \
            and "s2_semi" in _lib.last_error()
        rv = L.ssw_align_batch_active_ex(model_a._m, SEMI, d_in, 1, None, None, None, None, None,
                                         None, None, None, None, None, None)
        assert rv == -1 and "ssw_align_batch_active" in _lib.last_error() \
            and "s2_semi" in _lib.last_error()
        # and a model of 42 codebooks is not this scorer's, nor a single codebook PTM's
        with pytest.raises(ssw.SswError, match="codebooks"):
            gpu_en.score_batch(np.zeros((2, 39), np.float32), scorer=SEMI)
        with pytest.raises(ssw.SswError, match="single-codebook"):
            model_a.score_batch(feats_a[:2], scorer=ssw.SCORER_PTM)
    finally:
        model_a.device_free(d_in)


def test_a_nan_row(model_a, feats_a, restated_a):
    """a NaN feature: the call returns, the utterances beside it are the restatement's, the row
    itself is the same on every call"""
    off, reset, _, _ = restated_a
    bad = feats_a.copy()
    t = int(off[4]) + 5                      # inside the utterance of 64 frames
    bad[t, 7] = np.nan
    bad[t + 1, 38] = np.inf
    got = model_a.score_batch(bad, utt_off=off)
    assert np.array_equal(got[:off[4]], reset[:off[4]])
    assert np.array_equal(got[off[5]:], reset[off[5]:])
    assert np.array_equal(model_a.score_batch(bad, utt_off=off), got)


# ------------------------------------------------------------------------------------------
# the vtable object
# ------------------------------------------------------------------------------------------
def _delta_list(sens):
    """acmod_flags2list's uint8 delta list of ascending senones, with its bridge entries of 255"""
    out, last = [], 0
    for s in sens:
        d = s - last
        while d > 255:
            out.append(255)
            d -= 255
        out.append(d)
        last = s
    return np.array(out, np.uint8)


def test_vtable(model_a, feats_a, fx):
    g = ssw.S2SemiMgau(model_a)
    assert g.name == "s2_semi"
    assert g.transform() == -1
    want = model_a.score_batch(feats_a[:40])
    # 40 frames one at a time, as acmod calls: frame_idx is the next frame not yet scored
    for t in range(40):
        g.frame_idx = t
        assert np.array_equal(g.frame_eval(feats_a[t], t, compallsen=True), want[t]), t
    # an earlier frame (frame < frame_idx): its slot's row again
    g.frame_idx = 40
    assert np.array_equal(g.frame_eval(feats_a[39], 39), want[39])
    assert np.array_equal(g.frame_eval(feats_a[38], 38), want[38])
    # compallsen = 0: a delta list with a bridge entry (5 -> 700 is more than 255 apart)
    sens = [0, 5, 700, 701, 5125]
    lst = _delta_list(sens)
    assert 255 in lst.tolist()
    listed = np.cumsum(lst.astype(np.int64))
    g.reset_hist()
    for t in range(40):
        g.frame_idx = t
        row = g.frame_eval(feats_a[t], t, compallsen=False, senone_active=lst)
        assert np.array_equal(row[listed], want[t][listed]), t
        rest = np.ones(model_a.n_sen, bool)
        rest[listed] = False
        assert not row[rest].any(), t
    # reset_hist: frame 0 starts from the reset order again (the carried one gives other rows
    # only where scores tie, so the check is on the documented behaviour: the rows of a fresh
    # utterance)
    g.reset_hist()
    g.frame_idx = 0
    assert np.array_equal(g.frame_eval(feats_a[0], 0), want[0])
    # prescore: one batch, frame_eval copies its rows
    g.reset_hist()
    g.prescore(feats_a)
    g.frame_idx = 0
    _check_rows(np.stack([g.frame_eval(feats_a[t], t) for t in range(len(feats_a))]),
                fx["scoring"]["A"])
    g.free()


def test_vtable_ds(dirs, feats_a, fx):
    """the frame's own number decides whether a ds > 1 model scans the codebook"""
    m = ssw.Model(dirs["A"], config={"ds": 3})
    g = ssw.S2SemiMgau(m)
    want = m.score_batch(feats_a[:12])
    for t in range(12):
        g.frame_idx = t
        assert np.array_equal(g.frame_eval(feats_a[t], t), want[t]), t
    g.free()


# ------------------------------------------------------------------------------------------
# end to end on model A
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lex_a(model_a, dirs):
    return ssw.Lexicon(model_a, os.path.join(dirs["A"], "dict.txt"),
                       os.path.join(dirs["A"], "noisedict.txt"))


def _pcm():
    return np.fromfile(os.path.join(S.GOLD, "goforward.raw"), dtype="<i2")


def _rec_record(r, u):
    return {"hyp": r.hyp(u), "score": r.score(u), "segments": [list(s) for s in r.segments(u)],
            "json": r.json(u)}


def _rec_expected(rec):
    return {"hyp": rec["hyp"], "score": rec["score"], "segments": [s[:5] for s in rec["segments"]],
            "json": rec["json"]}


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
@pytest.mark.parametrize("grammar", ["goforward", "loop", "nulls"])
def test_recognize_audio_batch(model_a, lex_a, fx, grammar, active):
    pcm = _pcm()
    fsg = ssw.Fsg.read(model_a, lex_a, os.path.join(S.GOLD, "fsg", grammar + ".fsg"))
    plan = lex_a.grammar_plan(fsg)
    before = model_a.grammar_active_stats()
    r = ssw.recognize_audio_batch(model_a, lex_a, pcm, [0, len(pcm)], plan, active=active)
    assert r.status(0) == 0, r.message(0)
    assert _rec_record(r, 0) == _rec_expected(fx["rec"][grammar]["yes" if not active else "no"])
    if active:  # one round, everything accepted
        after = model_a.grammar_active_stats()
        assert (after[0] - before[0], after[1] - before[1], after[2], after[3] - before[3]) \
            == (1, 1, 1, 0)
    r.free()


def test_recognize_through_a_large_grammar_plan(model_a, lex_a, fx):
    pcm = _pcm()
    fsg = ssw.Fsg.read(model_a, lex_a, os.path.join(S.GOLD, "fsg", "goforward.fsg"))
    plan = lex_a.grammar_plan(fsg, max_hmms=30000)
    r = ssw.recognize_audio_batch(model_a, lex_a, pcm, [0, len(pcm)], plan)
    assert _rec_record(r, 0) == _rec_expected(fx["rec"]["goforward"]["yes"])
    r.free()


@pytest.mark.parametrize("active", [False, True], ids=["compallsen", "default"])
def test_align_audio_batch(model_a, lex_a, fx, active):
    pcm = _pcm()
    cfg = lex_a.first_pass_config(two_pass_history=1)
    before = model_a.first_pass_active_stats()
    a = ssw.align_audio_batch(model_a, lex_a, pcm, [0, len(pcm)],
                              ["go forward ten meters".split()], cfg=cfg, active=active)
    assert a.status(0) == 0, a.message(0)
    assert a.json(0).rstrip("\n") == fx["align"]["no" if active else "yes"]["json"].rstrip("\n")
    if active:
        after = model_a.first_pass_active_stats()
        assert (after[0] - before[0], after[1] - before[1], after[2], after[3] - before[3]) \
            == (1, 1, 1, 0)
    a.free()


def test_first_pass_batch_active_takes_the_whole_row_route(model_a, lex_a, feats_a):
    words = ["go forward ten meters".split()]
    d = model_a.to_device(feats_a)
    d_scr = model_a.to_device(model_a.score_batch(feats_a))
    try:
        want = lex_a.first_pass(d_scr, [0, len(feats_a)], words)
        got, rounds = lex_a.first_pass_active(d, [0, len(feats_a)], words)
        assert got == want and got[0] is not None and rounds.tolist() == [1]
        with pytest.raises(ssw.SswError, match="s2_semi"):
            lex_a.first_pass_active(d, [0, len(feats_a)], words, want_seed=True)
    finally:
        model_a.device_free(d)
        model_a.device_free(d_scr)
