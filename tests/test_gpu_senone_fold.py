"""ptm_senone_kernel's folded log-add chain (csrc/ssw_k1b_senone.inc, ssw_senone_lds.inc).

A chain step is x + H[x - y], H one byte per entry, instead of min(x, y) - tab[|x - y|]; the
weight byte is subtracted where it lies in the gathered dword.  The folded form can differ from
the reference only where d = x - y is at the ends of its reach or 0, so beside the shipped
models at the two batch sizes that take different instances (one and two frames per workgroup,
utterance starts inside the batch, an odd last unit) a model with weights 0 and 255 side by side
is scored on frames whose top-4 scores tie and on frames whose scores lie 96 or more apart.

No helper of the tests writes an mdef, so that model is not a tiny one: it is en-us's mdef, means
and variances under an 8-bit sendump made here (tests/sc_common.py:write_sendump8), its weights 0
and 255 by the parity of senone + density, in whole runs, or drawn from {0, 255} and from 0..255.
en-us's slot layout has short quads (runs of ids that are no multiple of 4) as it stands.  The
same extremes on made-up top-N blocks, the ms accumulator's start below zero and the Hb > 255
refusal are driven on the CPU by tests/test_senone_fold_host.py.

Everything is bit-exact against the CPU oracle (oracle/oracle.py)."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.synth import synth_features
from tests import sc_common as S
from tests.conftest import MODEL_ROOT
from tests.test_cabi_host import synth_mixw_from_sendump
from tests.test_gpu_logadd_negative import _near_tie_features

pytestmark = pytest.mark.gpu

KNOBS = [{}, {"SSW_SEN_GENERIC": "1"}, {"SSW_SEN_FPB": "1"}]
KNOB_IDS = ["default", "generic", "fpb1"]
BATCHES = {"2049": (700, 1, 648, 700), "130": (60, 1, 69)}

_REF = {}


def _batch(means, lens, seed):
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    feats = np.concatenate([synth_features(means, n, seed + i) for i, n in enumerate(lens)])
    return feats, off


def _ptm_reference(key, orc, feats, off):
    """the oracle's rows, once per batch, shared by the knob variants"""
    if key not in _REF:
        ref = np.concatenate([orc.ptm_score_utt(feats[off[i]:off[i + 1]])
                              for i in range(len(off) - 1)])
        ref.setflags(write=False)
        _REF[key] = ref
    return _REF[key]


def _set(monkeypatch, knobs):
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
@pytest.mark.parametrize("batch", list(BATCHES))
def test_en_us_both_batch_sizes(gpu_en, orc_en, means_en, monkeypatch, batch, knobs):
    """2,049 frames: two frames per group, the last unit one frame short; 130: one per group"""
    _set(monkeypatch, knobs)
    feats, off = _batch(means_en, BATCHES[batch], 6100)
    assert len(feats) == int(batch)
    ref = _ptm_reference(("en", batch), orc_en, feats, off)
    got = gpu_en.score_batch(feats, off)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, bad[:8].tolist()


# ---------------------------------------------------------------------------------------------
# weights 0 and 255 side by side
# ---------------------------------------------------------------------------------------------
def _extreme_weights(n_feat, n_density, n_sen):
    rng = np.random.default_rng(20261021)
    s = np.arange(n_sen)[None, None, :]
    d = np.arange(n_density)[None, :, None]
    f = np.arange(n_feat)[:, None, None]
    w = np.zeros((n_feat, n_density, n_sen), np.uint8)
    kind = np.broadcast_to((s // 64) % 5, w.shape)
    parity = np.broadcast_to((255 * ((s + d + 0 * f) & 1)).astype(np.uint8), w.shape)
    runs = np.broadcast_to((255 * ((s // 8 + 0 * d + 0 * f) & 1)).astype(np.uint8), w.shape)
    two = (255 * rng.integers(0, 2, w.shape)).astype(np.uint8)
    anyb = rng.integers(0, 256, w.shape, dtype=np.uint8)
    w[kind == 0] = parity[kind == 0]        # 0 | 255 in a pair, swapping with the codeword
    w[kind == 1] = runs[kind == 1]          # 8 slots of 0, 8 of 255: d = 0 in both halves
    w[kind == 2] = two[kind == 2]
    w[kind == 3] = anyb[kind == 3]
    w[kind == 4] = 0                        # equal weights whatever the codeword
    return w


@pytest.fixture(scope="module")
def extreme_models(oracle_mod, orc_en, tmp_path_factory):
    src = os.path.join(MODEL_ROOT, "en-us")
    sd = str(tmp_path_factory.mktemp("fold") / "sendump8")
    mixw = _extreme_weights(orc_en.n_feat, orc_en.n_density, orc_en.n_sen)
    S.write_sendump8(sd, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"), sendump=sd,
              tmat=os.path.join(src, "transition_matrices"))
    g = ssw.Model(variances=os.path.join(src, "variances"), **kw)
    o = oracle_mod.Model(vars=os.path.join(src, "variances"), **kw)
    assert np.array_equal(g.table("ptm_mixw").reshape(mixw.shape), mixw)
    return g, o


def _extreme_features(means):
    """ties first (frames half-way between two densities of a codebook), then frames far from
    every density (their top-4 scores lie more than 96 apart), then ordinary ones"""
    tie = _near_tie_features(means, 40, 15)
    far = (synth_features(means, 24, 16) * np.float32(8.0)).astype(np.float32)
    return np.ascontiguousarray(np.concatenate([tie, far, synth_features(means, 32, 17)]))


def test_the_extremes_occur(extreme_models, means_en):
    """the oracle's own chains on these inputs reach d = wmax = 255, d = 0 in two neighbouring
    slots at once and d <= -(255 + 96): recomputed in numpy from the oracle's top-N block, the
    restatement checked against the oracle's rows"""
    g, o = extreme_models
    feats = _extreme_features(means_en)[:64]
    out, cw, sc = o.ptm_score_utt(feats, want_topn=True)
    mixw = g.table("ptm_mixw").reshape(o.n_feat, o.n_density, o.n_sen).astype(np.int64)
    tab = np.concatenate([o.logadd_table_8b.astype(np.int64), np.zeros(1024, np.int64)])
    sen2cb = o.sen2cimap
    sen = np.arange(o.n_sen)
    n_max = n_zero2 = n_low = n_clamp = 0
    for t in range(len(feats)):
        q = sc[t].reshape(-1, o.n_feat, 4)
        c = cw[t].reshape(-1, o.n_feat, 4)
        tot = np.zeros(o.n_sen, np.int64)
        for f in range(o.n_feat):
            x = mixw[f, c[sen2cb, f, 0], sen] + q[sen2cb, f, 0]
            for k in range(1, 4):
                y = mixw[f, c[sen2cb, f, k], sen] + q[sen2cb, f, k]
                d = x - y
                n_max += int((d == 255).sum())
                n_low += int((d <= -(255 + 96)).sum())
                both = (d[:-1] == 0) & (d[1:] == 0) & (sen2cb[:-1] == sen2cb[1:])
                n_zero2 += int(both.sum())
                n_clamp += int((q[:, f, k] - q[:, f, 0] >= 96).sum())
                x = np.minimum(x, y) - tab[np.abs(d)]
            tot += x
        assert np.array_equal((tot - tot.min()).astype(np.int16), out[t])
    assert n_max > 100 and n_zero2 > 100 and n_low > 100 and n_clamp > 100, \
        (n_max, n_zero2, n_low, n_clamp)


@pytest.mark.parametrize("knobs", KNOBS[:2], ids=KNOB_IDS[:2])
def test_weights_0_and_255_side_by_side(extreme_models, means_en, monkeypatch, knobs):
    _set(monkeypatch, knobs)
    g, o = extreme_models
    feats = _extreme_features(means_en)
    off = np.array([0, 40, 41, len(feats)], np.int32)
    ref = _ptm_reference(("extreme",), o, feats, off)
    got = g.score_batch(feats, off)
    bad = np.argwhere(got != ref)
    assert len(bad) == 0, bad[:8].tolist()


# ---------------------------------------------------------------------------------------------
# the ms packed instance
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fr_ms_models(oracle_mod, orc_fr, tmp_path_factory):
    src = os.path.join(MODEL_ROOT, "fr-fr")
    mixw = str(tmp_path_factory.mktemp("foldms") / "mixture_weights")
    synth_mixw_from_sendump(orc_fr, mixw)
    kw = dict(mdef=os.path.join(src, "mdef"), means=os.path.join(src, "means"),
              tmat=os.path.join(src, "transition_matrices"), mixw=mixw)
    return (ssw.Model(variances=os.path.join(src, "variances"), **kw),
            oracle_mod.Model(vars=os.path.join(src, "variances"), **kw))


@pytest.mark.parametrize("knobs", KNOBS, ids=KNOB_IDS)
def test_ms_packed_instance_fr_fr(fr_ms_models, means_fr, monkeypatch, knobs):
    """2,049 frames through the ms scorer: the packed instance.  The oracle scores every frame
    on its own: the first 96 frames, those around the utterance starts and the odd last unit
    stand for it."""
    _set(monkeypatch, knobs)
    g, o = fr_ms_models
    feats, off = _batch(means_fr, (1024, 1, 1024), 6400)
    pick = np.r_[0:96, 1020:1030, 2045:2049]
    if ("ms",) not in _REF:
        ref = o.ms_score_utt(feats[pick])
        ref.setflags(write=False)
        _REF[("ms",)] = ref
    got = g.score_batch(feats, off, scorer=ssw.SCORER_MS)
    assert (got.min(axis=1) == 0).all()
    bad = np.argwhere(got[pick] != _REF[("ms",)])
    assert len(bad) == 0, bad[:8].tolist()
