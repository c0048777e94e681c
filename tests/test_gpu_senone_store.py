"""The senone kernels' output path under both slot layouts (csrc/ssw_slot_layout.inc).

With the prefix layout a quad holds n = 1..4 consecutive senone ids and ptm_senone_kernel writes
it with an 8-byte, a 4-byte and / or a 2-byte store; with SSW_SLOT_LAYOUT=dense a quad may
straddle two runs of ids and is written slot by slot.  A store that is too wide, or lands on a
neighbour's id, shows only in the rows themselves: every call here scores into a buffer with a
guard row before and behind the batch's rows, all of it pre-filled with a value no score takes,
and the rows are compared with the CPU oracle, the two layouts with each other.

Batches below 2,048 frames take one frame per workgroup, larger ones two (launch_senone), and
only those reach the packed ms instance: hence the 2,049-frame cases beside the small ones (an
odd last unit, rotating LDS slots with SSW_SEN_GROUPS=2)."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_alignment_task, synth_features
from tests.conftest import MODEL_ROOT
from tests.test_cabi_host import synth_mixw_from_sendump

pytestmark = pytest.mark.gpu

SENTINEL = -12345           # scores are `score - best` >= 0 (src/ptm_mgau.c:394-400, ms_mgau.c:314-320)
SMALL = [(1,), (2,), (3,), (5,), (7, 7)]
LAYOUTS = ("prefix", "dense")


def _load(layout, *args, **kw):
    """A model uploaded under the given slot layout (the knob is read when the model is loaded)."""
    old = os.environ.pop("SSW_SLOT_LAYOUT", None)
    if layout == "dense":
        os.environ["SSW_SLOT_LAYOUT"] = "dense"
    try:
        return ssw.Model(*args, **kw)
    finally:
        os.environ.pop("SSW_SLOT_LAYOUT", None)
        if old is not None:
            os.environ["SSW_SLOT_LAYOUT"] = old


@pytest.fixture(scope="module")
def en_models():
    return {lay: _load(lay, os.path.join(MODEL_ROOT, "en-us")) for lay in LAYOUTS}


@pytest.fixture(scope="module")
def fr_models(oracle_mod, orc_fr, tmp_path_factory):
    """fr-fr with a mixture_weights file (tests/test_gpu_ms.py): both scorers, and the oracle of
    the same files"""
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path_factory.mktemp("store") / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    g = {lay: _load(lay, variances=os.path.join(src, "variances"), **kw) for lay in LAYOUTS}
    return g, oracle_mod.Model(vars=os.path.join(src, "variances"), **kw)


_REF = {}


def _reference(key, orc, scorer, feats, off):
    """the oracle's rows, computed once per batch and shared by the variants that score it"""
    if key not in _REF:
        if scorer == ssw.SCORER_MS:
            ref = orc.ms_score_utt(feats)
        else:
            ref = np.concatenate([orc.ptm_score_utt(feats[off[i]:off[i + 1]])
                                  for i in range(len(off) - 1)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _batch(means, lens, seed):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    feats = np.concatenate([synth_features(means, n, seed + i) for i, n in enumerate(lens)])
    return feats, off


def _score_guarded(g, feats, off, scorer):
    """rows [n + 2][n_sen]: a guard row, the batch's rows, a guard row -- all pre-filled"""
    n = len(feats)
    buf = np.full((n + 2, g.n_sen), SENTINEL, np.int16)
    d_feats = g.to_device(feats)
    d_out = g.to_device(buf)
    try:
        g.score_batch_device(d_feats, n, off, d_out + 2 * g.n_sen, scorer=scorer)
        g._L.ssw_device_synchronize()
        g._L.ssw_memcpy_d2h(buf.ctypes.data, d_out, buf.nbytes)
    finally:
        g.device_free(d_feats)
        g.device_free(d_out)
    return buf


def _check_both_layouts(models, feats, off, scorer, ref, ref_rows=None):
    got = {}
    for lay in LAYOUTS:
        buf = _score_guarded(models[lay], feats, off, scorer)
        assert (buf[0] == SENTINEL).all(), (lay, "the guard row before the batch")
        assert (buf[-1] == SENTINEL).all(), (lay, "the guard row behind the batch")
        rows = buf[1:-1]
        left = np.argwhere(rows == SENTINEL)
        assert len(left) == 0, (lay, "entries never written (frame, senone)", left[:8].tolist())
        sel = slice(None) if ref_rows is None else ref_rows
        bad = np.argwhere(rows[sel] != ref)
        assert len(bad) == 0, (lay, "rows differ from the oracle at", bad[:8].tolist())
        got[lay] = rows
    assert got["prefix"].tobytes() == got["dense"].tobytes()


@pytest.mark.parametrize("groups", ["0", "2"])
@pytest.mark.parametrize("lens", SMALL, ids=lambda l: "x".join(map(str, l)))
def test_ptm_en_us_small_batches(en_models, orc_en, means_en, monkeypatch, lens, groups):
    monkeypatch.setenv("SSW_SEN_GROUPS", groups)
    feats, off = _batch(means_en, lens, 4100)
    ref = _reference(("en", "ptm", lens), orc_en, ssw.SCORER_PTM, feats, off)
    _check_both_layouts(en_models, feats, off, ssw.SCORER_PTM, ref)


@pytest.mark.parametrize("groups", ["0", "2"])
@pytest.mark.parametrize("scorer", [ssw.SCORER_PTM, ssw.SCORER_MS], ids=["ptm", "ms"])
@pytest.mark.parametrize("lens", SMALL, ids=lambda l: "x".join(map(str, l)))
def test_fr_fr_small_batches(fr_models, means_fr, monkeypatch, lens, scorer, groups):
    monkeypatch.setenv("SSW_SEN_GROUPS", groups)
    g, orc = fr_models
    feats, off = _batch(means_fr, lens, 4200)
    ref = _reference(("fr", scorer, lens), orc, scorer, feats, off)
    _check_both_layouts(g, feats, off, scorer, ref)


@pytest.mark.parametrize("groups", ["0", "2"])
def test_ptm_en_us_two_frames_per_group(en_models, orc_en, means_en, monkeypatch, groups):
    """2,049 frames: the default instance (3 quads per thread, 2 frames per group), its last
    unit one frame short; two groups take 513 and 512 units through the rotating slots."""
    monkeypatch.setenv("SSW_SEN_GROUPS", groups)
    lens = (1024, 1025)
    feats, off = _batch(means_en, lens, 4300)
    ref = _reference(("en", "ptm", lens), orc_en, ssw.SCORER_PTM, feats, off)
    _check_both_layouts(en_models, feats, off, ssw.SCORER_PTM, ref)


@pytest.mark.parametrize("groups", ["0", "2"])
def test_ms_fr_fr_packed_instance(fr_models, means_fr, monkeypatch, groups):
    """2,049 frames through the ms scorer: the packed instance of ptm_senone_kernel.  The oracle
    scores every frame on its own, so the first 160 frames and the last 3 (the odd unit) stand
    for it; the layouts are compared over all rows."""
    monkeypatch.setenv("SSW_SEN_GROUPS", groups)
    g, orc = fr_models
    feats, off = _batch(means_fr, (2049,), 4400)
    pick = np.r_[0:160, 2046:2049]
    ref = _reference(("fr", "ms", "packed"), orc, ssw.SCORER_MS, feats[pick], None)
    _check_both_layouts(g, feats, off, ssw.SCORER_MS, ref, ref_rows=pick)


def test_compact_rows_equal_the_full_rows(en_models, orc_en, means_en):
    """cpos is rebuilt from the layout's senone-to-slot map: three frames into compact rows, each
    state's column against its senone's entry of the full row, under both layouts."""
    lens, phones = [3], [2]
    feats, off = _batch(means_en, lens, 4500)
    senid, _, _ = synth_alignment_task(orc_en.sseq, orc_en.phone_ssid, orc_en.phone_tmat,
                                       orc_en.n_ciphone, phones[0], 4600)
    phone_off = np.array([0, phones[0]], np.int32)
    ref = _reference(("en", "ptm", "compact"), orc_en, ssw.SCORER_PTM, feats, off)
    ids = np.asarray(senid, np.uint16).reshape(-1).astype(np.int64)
    first = {}
    for k, s_ in enumerate(ids):
        first.setdefault(int(s_), k)
    cols = np.array([first[int(s_)] for s_ in ids])
    for lay in LAYOUTS:
        g = en_models[lay]
        d_feats = g.to_device(feats)
        plan = g.compact_plan(off, phone_off, senid)
        d_c = g.device_malloc(max(plan.nbytes, 2))
        try:
            g.score_batch_compact(d_feats, plan, d_c)
            g._L.ssw_device_synchronize()
            buf = np.zeros(plan.elems, np.int16)
            g._L.ssw_memcpy_d2h(buf.ctypes.data, d_c, buf.nbytes)
            o, stride = plan.rows(0)
        finally:
            g.device_free(d_feats)
            g.device_free(d_c)
            plan.free()
        rows = buf[o:o + lens[0] * stride].reshape(lens[0], stride)
        assert np.array_equal(rows[:, cols], ref[:, ids]), lay
