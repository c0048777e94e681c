"""GPU parity: dynamic features of every configuration (ssw_feat_batch_ex), bit-exact float32.

Every case recorded from the reference (tests/golden/feat_types, tests/feat_types_common.CASES):
tobytes() equality.  Ragged batches of every type and CMN mode against the numpy restatement,
which tests/test_feat_types_host.py shows to reproduce every recorded case.  The plain
configuration against ssw_feat_batch.  Live CMN's state along a chain of utterances.  Model
C1-lda recognised and aligned from PCM to the reference's strings."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from tests import cont_common as CC
from tests import feat_types_common as FT

pytestmark = pytest.mark.gpu

TYPES = ["s2_4x", "s3_1x39", "1s_c_d_dd", "1s_c_d_ld_dd", "cep_dcep", "cep", "1s_3c", "1s_4c",
         "13:2", "4,9:1"]
CMNS = {"none": dict(cmn="none"), "batch": dict(cmn="batch"),
        "varnorm": dict(cmn="batch", varnorm="yes"), "live": dict(cmn="live", cmninit=FT.INIT13)}


@pytest.fixture(scope="module")
def fx():
    return FT.cases()


def _feat(model, settings):
    kw = dict(FT.DEFAULTS, **settings)
    kw["varnorm"] = str(kw["varnorm"]).lower() in ("yes", "true", "1")
    return model.feat(**kw)


def _state(feat, tup):
    s = ssw.SswCmnState()
    n = len(tup[0])
    s.mean[:n] = tup[0].tolist()
    s.sum[:n] = tup[1].tolist()
    s.nframe = int(tup[2])
    return s


def _same_state(s, tup, n):
    got = FT.state_tuple(s)
    return (got[0][:n].tobytes() == np.asarray(tup[0], np.float32).tobytes()
            and got[1][:n].tobytes() == np.asarray(tup[1], np.float32).tobytes() and got[2] == int(tup[2]))


@pytest.mark.parametrize("name", sorted(FT.CASES))
def test_recorded_case(gpu_en, fx, name):
    c = fx[name]
    feat = _feat(gpu_en, c["settings"])
    assert feat.out_dim == c["dims"]["width"]
    cep, off = FT.case_input(c), FT.offsets(c["lens"])
    n = c["dims"]["ceplen"]
    state = feat.cmn_prior() if c["mode"] == "chain" else None
    got = gpu_en.feat_batch_ex(cep, off, feat, state)
    assert got.tobytes() == c["out"].tobytes(), name
    if state is not None:
        assert _same_state(state, (c["state"][-1, :n], c["state"][-1, n:], c["nframe"][-1]), n)
    feat.free()


def _ragged(tf, ncep, seed):
    """utterances of 1, 2, 3, 7, 300 and 5 frames, an empty one in the middle, and one of a tile
    less a frame, a tile, a tile and a frame; c0 >= 0 everywhere but in every fifth frame of the
    long one; seeded random cepstra (no dimension of an utterance is constant)"""
    rng = np.random.default_rng(seed)
    lens = [1, 2, 3, 0, 7, 300, 5, tf - 1, tf, tf + 1]
    ceps = [rng.normal(0, 4, (n, ncep)).astype(np.float32) for n in lens]
    for c in ceps:
        c[:, 0] = np.abs(c[:, 0])
    ceps[5][::5, 0] = -1.0
    return np.concatenate(ceps), FT.offsets(lens)


def _same_but_nan_signs(got, want):
    """byte equality, except that where BOTH hold a NaN its sign and payload are not compared:
    a one-frame utterance under varnorm is 0 * inf in every dimension"""
    g, w = got.view(np.uint32).copy(), want.view(np.uint32).copy()
    both = np.isnan(got) & np.isnan(want)
    g[both] = w[both] = 0x7fc00000
    return g.tobytes() == w.tobytes()


@pytest.mark.parametrize("cmn", sorted(CMNS))
@pytest.mark.parametrize("ftype", TYPES)
def test_ragged_batch_against_the_restatement(gpu_en, ftype, cmn):
    settings = dict(CMNS[cmn], feat=ftype)
    feat = _feat(gpu_en, settings)
    cep, off = _ragged(feat.tile_frames, 13, 7)
    want, _ = FT.restate(cep, off, settings)
    got = gpu_en.feat_batch_ex(cep, off, feat)
    assert got.shape == want.shape
    if cmn == "varnorm":
        assert np.isnan(want[0]).all() and not np.isnan(want[1:]).any()
        assert _same_but_nan_signs(got, want)
    else:
        assert got.tobytes() == want.tobytes()
    feat.free()


@pytest.mark.parametrize("name,settings", [
    ("lda_29", dict(cmn="batch", lda=FT.LDA_FILE, ldadim=29)),
    ("lda_live", dict(lda=FT.LDA_FILE)),
    ("lda_sv", dict(cmn="batch", varnorm="yes", lda=FT.LDA_FILE, ldadim=20, svspec="19,0-8/9-17,30")),
    ("sv", dict(cmn="none", svspec="24,0-11/25,12-23/26-38")),
    ("ceplen_20", dict(cmn="batch", feat="1s_c_d_ld_dd", ceplen=20)),
    ("ceplen_64_w8", dict(cmn="batch", varnorm="yes", feat="30,34:8", ceplen=64)),
])
def test_ragged_batch_with_projections_and_other_widths(gpu_en, name, settings):
    feat = _feat(gpu_en, settings)
    cep, off = _ragged(feat.tile_frames, feat.ceplen, 11)
    want, _ = FT.restate(cep, off, settings)
    got = gpu_en.feat_batch_ex(cep, off, feat)
    assert got.shape == want.shape
    if "varnorm" in settings:
        assert _same_but_nan_signs(got, want)
    else:
        assert got.tobytes() == want.tobytes()
    feat.free()


def test_plain_configuration_is_feat_batch(gpu_en):
    feat = gpu_en.feat()                 # en-us: 1s_c_d_dd, cmn current, svspec 0-12/13-25/26-38
    assert gpu_en.feat_plain() and feat.out_dim == 39
    cep, off = _ragged(feat.tile_frames, 13, 3)
    assert gpu_en.feat_batch_ex(cep, off).tobytes() == gpu_en.feat_batch(cep, off).tobytes()
    m = FT.mfcc()
    assert gpu_en.feat_batch_ex(m).tobytes() == gpu_en.feat_batch(m).tobytes()
    assert gpu_en.feat_batch_ex(np.zeros((0, 13), np.float32)).shape == (0, 39)


def test_live_chain_in_one_call_and_in_three(gpu_en, fx):
    c = fx["chain"]
    feat = _feat(gpu_en, c["settings"])
    cep, off = FT.case_input(c), FT.offsets(c["lens"])
    one = feat.cmn_prior()
    got = gpu_en.feat_batch_ex(cep, off, feat, one)
    assert got.tobytes() == c["out"].tobytes()
    s = feat.cmn_prior()
    parts = []
    for u in range(3):
        parts.append(gpu_en.feat_batch_ex(cep[off[u]:off[u + 1]], None, feat, s))
        assert _same_state(s, (c["state"][u, :13], c["state"][u, 13:], c["nframe"][u]), 13), u
    assert np.concatenate(parts).tobytes() == got.tobytes()
    assert bytes(one) == bytes(s)
    # without a state every utterance is a fresh decoder's first
    fresh = gpu_en.feat_batch_ex(cep, off, feat)
    assert fresh[:200].tobytes() == got[:200].tobytes() and fresh[200:].tobytes() != got[200:].tobytes()
    # batch and none neither read nor write the state
    for cmn in ("batch", "none"):
        f2 = _feat(gpu_en, dict(cmn=cmn))
        before = bytes(s)
        assert gpu_en.feat_batch_ex(cep, off, f2, s).tobytes() == gpu_en.feat_batch_ex(cep, off, f2).tobytes()
        assert bytes(s) == before
        f2.free()
    feat.free()


def test_live_state_at_the_window_edges(gpu_en):
    """cmn_live's shift asks nframe >= 800 (after > 800 let it in), cmn_live_update nframe > 800:
    a state of exactly 800 frames decays in neither through an empty utterance, one of 801 does;
    799 + 2 frames takes the shift"""
    feat = _feat(gpu_en, {})
    rng = np.random.default_rng(5)
    cep = np.abs(rng.normal(0, 4, (2, 13))).astype(np.float32)
    total = rng.normal(0, 3000, 13).astype(np.float32)
    for nframe, lens in ((800, [0]), (801, [0]), (799, [2]), (799, [1]), (0, [0]), (0, [2])):
        tup = ((total / np.float32(max(nframe, 1))).astype(np.float32), total, nframe)
        off = FT.offsets(lens)
        want, states = FT.restate(cep[:off[-1]], off, {}, tup)
        s = _state(feat, tup)
        got = gpu_en.feat_batch_ex(cep[:off[-1]], off, feat, s)
        assert got.tobytes() == want.tobytes(), (nframe, lens)
        assert _same_state(s, states[-1], 13), (nframe, lens)
    feat.free()


# ------------------------------------------------------------------------------------------
# end to end on C1-lda
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def c1_lda(tmp_path_factory):
    d = FT.model_c1_lda_dir(str(tmp_path_factory.mktemp("c1lda") / "C1-lda"))
    m = ssw.Model(**CC.model_paths(d))
    lex = ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    yield m, lex
    m.close()


def _pcm():
    return np.fromfile(os.path.join(CC.GOLD, "goforward.raw"), dtype="<i2")


def test_c1_lda_is_recognised_and_aligned_from_pcm(c1_lda):
    m, lex = c1_lda
    e = FT.e2e()
    assert not m.feat_plain() and m.feat().out_dim == 32 == m.veclen_total
    pcm = _pcm()
    plan = lex.grammar_plan(ssw.Fsg.read(m, lex, os.path.join(CC.GOLD, "fsg", "goforward.fsg")))
    r = ssw.recognize_audio_batch(m, lex, pcm, [0, len(pcm)], plan)
    assert r.status(0) == 0, r.message(0)
    rec = e["rec"]
    assert {"hyp": r.hyp(0), "score": r.score(0), "segments": [list(s) for s in r.segments(0)],
            "json": r.json(0)} \
        == {"hyp": rec["hyp"], "score": rec["score"], "segments": [s[:5] for s in rec["segments"]],
            "json": rec["json"]}
    r.free()
    a = ssw.align_audio_batch(m, lex, pcm, [0, len(pcm)], ["go forward ten meters".split()])
    assert a.status(0) == 0, a.message(0)
    assert a.json(0).rstrip("\n") == e["align"]["json"].rstrip("\n")
    a.free()


def test_a_transform_of_another_width_is_refused_with_both(tmp_path):
    """the real 36-row matrix beside 39-dimensional means"""
    d = FT.model_c1_lda_dir(str(tmp_path / "C1-36"), matrix=FT.read_lda(FT.LDA_FILE), permute=False)
    m = ssw.Model(**CC.model_paths(d))
    lex = ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    pcm = _pcm()
    with pytest.raises(ssw.SswError, match="rows of 36 floats, but its Gaussians' streams are 39 wide"):
        ssw.align_audio_batch(m, lex, pcm, [0, len(pcm)], ["go forward ten meters".split()])
    plan = lex.grammar_plan(ssw.Fsg.read(m, lex, os.path.join(CC.GOLD, "fsg", "goforward.fsg")))
    with pytest.raises(ssw.SswError, match="rows of 36 floats, but its Gaussians' streams are 39 wide"):
        ssw.recognize_audio_batch(m, lex, pcm, [0, len(pcm)], plan)
    m.close()


# ------------------------------------------------------------------------------------------
# refusals through the C ABI
# ------------------------------------------------------------------------------------------
def test_refusals(gpu_en):
    cep = np.zeros((4, 12), np.float32)
    with pytest.raises(ssw.SswError, match="12 cepstra per frame, but the configuration's ceplen is 13"):
        gpu_en.feat_batch_ex(cep)
    with pytest.raises(ssw.SswError, match=r"LDA incompatible with multi-stream features \(n_stream = 4\)"):
        gpu_en.feat(feat="s2_4x", svspec=None, lda=FT.LDA_FILE)
    with pytest.raises(ssw.SswError, match="Variance normalization not implemented in live mode"):
        gpu_en.feat(cmn="live", varnorm=True)
    with pytest.raises(ssw.SswError, match="utt_off must run from 0 to n_frames"):
        gpu_en.feat_batch_ex(np.zeros((4, 13), np.float32), [0, 3, 2, 4])
    other = ssw.Model(ssw.model_dir("fr-fr"), config={"device": ssw.SSW_DEVICE_NONE})
    with pytest.raises(ssw.SswError, match="created for another model"):
        gpu_en.feat_batch_ex(np.zeros((4, 13), np.float32), None, other.feat())
    other.close()
