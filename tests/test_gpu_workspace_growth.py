"""Grow and reuse of every grow-only device workspace of a model (devbuf_reserve,
csrc/ssw_host_model.inc), one case per buffer.

The session-wide models of conftest.py have whatever workspace sizes earlier tests left them, so
every case LOADS ITS OWN model and runs one entry point three times on it: a small batch (2
utterances of 24 and 40 frames), a larger one (9 utterances of 30 to 120 frames: every buffer
grows), the small one again (every buffer is reused, too big).  Each result is compared bit for
bit with the same call on a freshly loaded model, whose buffers have exactly that call's size.
Features are cut from tests/golden/goforward_mfcc.npy; what a cut utterance aligns or recognises
to does not matter here, only that it is what a fresh model gives.

The cached-graphs branches are taken where the same graphs are searched twice in a row: a
FirstPassPlan run on two recordings (ssw_align_text_batch builds new graphs on every call, so it
never takes that branch itself), and a grammar plan searched again after another plan was.

d_full_tmp: ssw_score_batch_compact's full-rows fall-back is what every ms launch of fewer than
2,048 frames takes (ms_takes_packed_kernel), so the small shapes reach it with the ms scorer."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_alignment_task
from tests import fsg_common as FC
from tests.conftest import MODEL_ROOT, ROOT

pytestmark = pytest.mark.gpu

SMALL = [24, 40]
LARGE = [30, 41, 52, 63, 75, 86, 97, 108, 120]
GOLD = os.path.join(ROOT, "tests", "golden")


class Ctx:
    """a freshly loaded model with its lexicon"""

    def __init__(self, name="en-us", **kw):
        d = os.path.join(MODEL_ROOT, name)
        self.m = ssw.Model(**kw) if kw else ssw.Model(d)
        self.lex = ssw.Lexicon(self.m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
        self.plans, self.fsgs = {}, {}

    def close(self):
        for x in list(self.plans.values()) + list(self.fsgs.values()):
            x.free()
        self.lex.free()
        self.m.close()


@pytest.fixture(scope="module")
def f39():
    """the recording's 39-dimensional features, once"""
    c = Ctx()
    try:
        cep = np.load(os.path.join(GOLD, "goforward_mfcc.npy")).astype(np.float32)
        return np.ascontiguousarray(c.m.feat_batch(cep), np.float32)
    finally:
        c.close()


def _batch(f39, lens, start=40, step=0):
    """utterance i: lens[i] frames from frame start + i * step on ("go" begins at frame 46)"""
    parts = [f39[(start + i * step) % (len(f39) - n):][:n] for i, n in enumerate(lens)]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    return np.ascontiguousarray(np.concatenate(parts)), off


def _texts(lens):
    return [["go"] if n < 88 else ["go", "forward"] for n in lens]


def _aset_record(aset, n_utts):
    out = []
    for u in range(n_utts):
        a = aset.utterance(u)
        out.append((aset.status(u), aset.message(u),
                    None if a is None else {k: np.asarray(v).tolist() for k, v in a.items()}))
    aset.free()
    return out


def _rset_record(r):
    out = [(r.status(u), r.message(u), r.hyp(u), r.score(u), r.segments(u)) for u in range(len(r))]
    r.free()
    return out


def _grow_and_reuse(load, run, order=("small", "large", "small")):
    """run(ctx, which) on one model in `order`; each result against the same call on a fresh model"""
    a = load()
    fresh = {}
    try:
        for i, which in enumerate(order):
            got = run(a, which)
            if which not in fresh:
                b = load()
                try:
                    fresh[which] = run(b, which)
                finally:
                    b.close()
            assert got == fresh[which], (i, which)
    finally:
        a.close()
    return fresh


def test_carried_orders(f39):
    """d_carry0: ssw_score_batch_ex with carry_in"""
    def run(c, which):
        feats, off = _batch(f39, SMALL if which == "small" else LARGE, step=7)
        cin = np.full(c.m.n_cb * c.m.n_feat, 0x00010203, np.uint32)
        scr, cout = c.m.score_batch_carry(feats, off, carry_in=cin)
        return scr.tobytes(), cout.tobytes()
    _grow_and_reuse(Ctx, run)


@pytest.mark.parametrize("two_pass", [0, 1])
def test_align_text_batch(f39, two_pass):
    """d_text_scr, d_carry_rows (two_pass_history), d_fp_ws, d_align_ws"""
    def run(c, which):
        lens = SMALL if which == "small" else LARGE
        feats, off = _batch(f39, lens)
        d = c.m.to_device(feats)
        try:
            aset = ssw.align_text_batch(c.m, c.lex, d, off, _texts(lens),
                                        cfg=c.lex.first_pass_config(two_pass_history=two_pass))
            return _aset_record(aset, len(lens))
        finally:
            c.m.device_free(d)
    fresh = _grow_and_reuse(Ctx, run)
    n_ok = sum(r[0] == 0 for r in fresh["small"] + fresh["large"])
    print("aligned:", n_ok, "of", len(SMALL) + len(LARGE))


def test_first_pass_plan_on_two_recordings(f39):
    """d_fp_ws with the graphs cached: one plan's texts searched on a small-score recording, then
    (the same graphs: only the call's tables go up) on other recordings, after the workspace grew
    for another plan in between -- against a fresh model, which uploads everything"""
    def run(c, which):
        lens = SMALL if which.startswith("small") else LARGE
        feats, off = _batch(f39, lens, start=38 if which.endswith("again") else 40)
        key = "small" if which.startswith("small") else "large"
        if key not in c.plans:
            c.plans[key] = ssw.FirstPassPlan(c.m, c.lex, _texts(lens))
        d = c.m.to_device(c.m.score_batch(feats, off))
        try:
            return _aset_record(ssw.forced_align_planned(c.m, c.lex, c.plans[key], d, off), len(lens))
        finally:
            c.m.device_free(d)
    # small (miss), small again (hit), large (miss: grown), large again (hit), small (miss)
    _grow_and_reuse(Ctx, run, ("small", "small_again", "large", "large_again", "small"))


def test_default_configuration_text(f39):
    """d_fpa_ws, d_fp_ws (its rounds search the same graphs again: the cached branch), d_text_scr:
    ssw_align_text_batch_active and ssw_first_pass_batch_active"""
    def run(c, which):
        lens = SMALL if which == "small" else LARGE
        feats, off = _batch(f39, lens)
        d = c.m.to_device(feats)
        try:
            aset = ssw.align_text_batch_active(c.m, c.lex, d, off, _texts(lens))
            rec = _aset_record(aset, len(lens))
            segs, rounds = c.lex.first_pass_active(d, off, _texts(lens))
            return rec, segs, rounds.tolist()
        finally:
            c.m.device_free(d)
    _grow_and_reuse(Ctx, run)


@pytest.mark.parametrize("active", [False, True])
def test_grammar_plans_in_turn(f39, active):
    """d_gr_ws, d_text_scr (and d_fpa_ws with active): goforward.fsg on the small batch (the
    plan's graphs go up), loop50.fsg on the large one (the workspace grows and the cache is
    dropped), goforward.fsg again (another plan was searched in between: its graphs go up
    again), and once more on other features (the same plan twice in a row: only the call's
    tables go up)"""
    def run(c, which):
        if not c.plans:
            c.fsgs = {g: ssw.Fsg.read(c.m, c.lex, FC.fsg_path(g)) for g in ("goforward", "loop50")}
            c.plans = {g: c.lex.grammar_plan(f) for g, f in c.fsgs.items()}
        lens = SMALL if which.startswith("small") else LARGE
        plan = c.plans["goforward" if which.startswith("small") else "loop50"]
        feats, off = _batch(f39, lens, start=38 if which.endswith("again") else 40, step=5)
        d = c.m.to_device(feats)
        try:
            if active:
                r, rounds = ssw.recognize_batch_active(c.m, c.lex, d, off, plan)
                return _rset_record(r), rounds.tolist()
            return _rset_record(ssw.recognize_batch(c.m, c.lex, d, off, plan))
        finally:
            c.m.device_free(d)
    _grow_and_reuse(Ctx, run, ("small", "large", "small", "small_again"))


def _align_task(m, lens, seed):
    sseq = m.table("sseq").reshape(-1, 3)
    senid, tmat = [], []
    phones = [max(2, n // 8) for n in lens]
    for i, n in enumerate(phones):
        s, t, _ = synth_alignment_task(sseq, m.table("phone_ssid"), m.table("phone_tmat"),
                                       m.n_ciphone, n, seed + i)
        senid.append(s)
        tmat.append(t)
    phone_off = np.concatenate([[0], np.cumsum(phones)]).astype(np.int32)
    return phone_off, np.concatenate(senid), np.concatenate(tmat)


def test_align_batch_active(f39):
    """d_act_ws (and d_align_ws): ssw_align_batch_active"""
    def run(c, which):
        lens = SMALL if which == "small" else LARGE
        feats, off = _batch(f39, lens, step=11)
        phone_off, senid, tmat = _align_task(c.m, lens, 4200)
        d = c.m.to_device(feats)
        try:
            st, status = c.m.align_batch_active(d, off, phone_off, senid, tmat)
            return st.tobytes(), status.tolist()
        finally:
            c.m.device_free(d)
    _grow_and_reuse(Ctx, run)


def test_front_end_and_features():
    """d_fe_ws, d_feat_off: ssw_fe_batch and ssw_feat_batch on 0.3 s, then three cuts of up to
    1.2 s, of goforward.raw"""
    pcm = FC.pcm("goforward.raw", 0)

    def run(c, which):
        cuts = [pcm[:4800]] if which == "small" else [pcm[:19200], pcm[4800:14400], pcm[:4800]]
        cep, fo = c.m.fe_batch(cuts)
        return cep.tobytes(), fo.tolist(), c.m.feat_batch(cep, fo).tobytes()
    _grow_and_reuse(Ctx, run)


def test_compact_rows_through_the_full_row_fall_back(orc_fr, tmp_path):
    """d_full_tmp: ssw_score_batch_compact with the ms scorer on batches of fewer than 2,048
    frames (fr-fr with mixture weights made from its sendump, as tests/test_gpu_ms.py does)"""
    from tests.test_cabi_host import synth_mixw_from_sendump
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              variances=os.path.join(src, "variances"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    cep = np.load(os.path.join(GOLD, "goforward_fr_mfcc.npy")).astype(np.float32)
    feats_fr = []

    def run(c, which):
        if not feats_fr:
            feats_fr.append(np.ascontiguousarray(c.m.feat_batch(cep), np.float32))
        lens = SMALL if which == "small" else LARGE
        feats, off = _batch(feats_fr[0], lens, step=9)
        phone_off, senid, _ = _align_task(c.m, lens, 5200)
        plan = c.m.compact_plan(off, phone_off, senid)
        # (zeros first: a column whose senone an earlier state of the utterance has is not written)
        d, d_c = c.m.to_device(feats), c.m.to_device(np.zeros(max(plan.elems, 1), np.int16))
        try:
            c.m.score_batch_compact(d, plan, d_c, scorer=ssw.SCORER_MS)
            c.m._L.ssw_device_synchronize()
            buf = np.zeros(plan.elems, np.int16)
            c.m._L.ssw_memcpy_d2h(buf.ctypes.data, d_c, buf.nbytes)
            return buf.tobytes()
        finally:
            c.m.device_free(d)
            c.m.device_free(d_c)
            plan.free()
    _grow_and_reuse(lambda: Ctx("fr-fr", **kw), run)
