"""Dynamic features of every configuration, on the CPU: the numpy restatement
(tests/feat_types_common.py) reproduces every case recorded from the reference byte for byte --
only then is it a yardstick for the ragged batches of tests/test_gpu_feat_types.py --, the
configuration parser and ssw_feat_create's checks (defaults, aliases, the model directory's
feature_transform, the dimensions the reference reports, every refusal by its words), and the
tile table builder as a stand-alone program under ASan + UBSan."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from tests import feat_types_common as FT
from tests.conftest import MODEL_ROOT, ROOT

NONE = {"device": ssw.SSW_DEVICE_NONE}
EN_US = os.path.join(MODEL_ROOT, "en-us")
PLAIN = dict(feat="1s_c_d_dd", svspec=None, cmn="batch")


@pytest.fixture(scope="module")
def fx():
    return FT.cases()


@pytest.fixture(scope="module")
def model():
    _lib.build()
    m = ssw.Model(EN_US, config=NONE)
    yield m
    m.close()


def _settings(s):
    """a case's settings as Model.feat overrides over the reference's defaults"""
    kw = dict(FT.DEFAULTS, **s)
    kw["varnorm"] = str(kw["varnorm"]).lower() in ("yes", "true", "1")
    return kw


def test_fixture_holds_every_case(fx):
    assert sorted(fx) == sorted(FT.CASES)
    for name, c in fx.items():
        assert c["settings"] == FT.CASES[name]["settings"] and c["lens"] == FT.CASES[name]["lens"], name
        assert c["out"].shape == (sum(c["lens"]), c["dims"]["width"]), name
        assert ("state" in c) == bool(c["dims"]["has_cmn"]), name
    for f in ("types", "cmn", "lda", "chain"):
        assert os.path.getsize(os.path.join(FT.DIR, f + ".npz")) < os.path.getsize(
            os.path.join(FT.GOLD, "cont", "rows.npz")), f
    e = FT.e2e()
    assert e["rec"]["hyp"] == "go forward ten meters" and e["align"]["json"]


@pytest.mark.parametrize("name", sorted(FT.CASES))
def test_restatement_reproduces_the_reference(fx, name):
    c = fx[name]
    r = FT.resolve(c["settings"])
    assert (r["width"], r["raw"], r["window"], len(r["streams"]), r["ceplen"]) == tuple(
        c["dims"][k] for k in ("width", "raw", "window", "streams", "ceplen")), name
    out, states = FT.restate(FT.case_input(c), FT.offsets(c["lens"]), c["settings"],
                             r["prior"] if c["mode"] == "chain" else None)
    assert out.tobytes() == c["out"].tobytes(), name
    if "state" in c:
        n = r["ceplen"]
        for u, (mean, total, nframe) in enumerate(states):
            assert mean.tobytes() == c["state"][u, :n].tobytes(), (name, u)
            assert total.tobytes() == c["state"][u, n:].tobytes(), (name, u)
            assert nframe == c["nframe"][u], (name, u)


def test_the_chain_cases_cross_the_window(fx):
    """the recorded chains take cmn_live's shift (nframe > 800 -> 500), and an empty utterance is
    given cmn_live_update alone"""
    assert list(fx["chain"]["nframe"]) == [700, 500, 600]
    assert list(fx["chain_empty"]["nframe"]) == [620, 620, 500, 540]
    s = fx["chain_empty"]["state"]
    assert s[0].tobytes() == s[1].tobytes()


def test_the_negc0_cases_skip_frames(fx):
    assert list(fx["negc0_batch"]["nframe"]) == [1, 1, 3, 3, 4, 7, 32]
    assert fx["negc0_batch"]["out"].tobytes() != fx["1s_c_d_dd"]["out"].tobytes()


# ---- the parser ------------------------------------------------------------------------------
def test_defaults_are_the_references(tmp_path):
    c = ssw.FeatConfig.read(None).as_dict()
    assert c == {"feat": "1s_c_d_dd", "ceplen": 13, "cmn": "live", "cmninit": "40,3,-1",
                 "varnorm": False, "lda": None, "ldadim": 0, "svspec": None, "from_file": False}
    p = tmp_path / "feat_params.json"
    p.write_text('{"-feat": "s2_4x", "cmn": "current", "varnorm": "yes", "ldadim": 7, "lda": null,\n'
                 ' "cmninit": "1,2", "svspec": "0-3", "ceplen": 13, "nfilt": 20, "lowerf": 1e2}')
    c = ssw.FeatConfig.read(str(p)).as_dict()
    assert c == {"feat": "s2_4x", "ceplen": 13, "cmn": "batch", "cmninit": "1,2", "varnorm": True,
                 "lda": None, "ldadim": 7, "svspec": "0-3", "from_file": True}
    assert ssw.FeatConfig.read(str(tmp_path / "none.json")).as_dict()["from_file"] is False


@pytest.mark.parametrize("alias,cmn", [("none", "none"), ("batch", "batch"), ("current", "batch"),
                                       ("live", "live"), ("prior", "live")])
def test_cmn_aliases(tmp_path, alias, cmn):
    p = tmp_path / "feat_params.json"
    p.write_text(json.dumps({"cmn": alias}))
    assert ssw.FeatConfig.read(str(p)).as_dict()["cmn"] == cmn


@pytest.mark.parametrize("body,words", [
    ('{"cmn": "sometimes"}', 'cannot use "sometimes" as the value of "cmn"'),
    ('{"ceplen": "many"}', 'cannot use "many" as the value of "ceplen"'),
    ('{"varnorm": "perhaps"}', 'cannot use "perhaps" as the value of "varnorm"'),
    ('["feat"]', "not a JSON object"),
    ('{"feat": "s2_4x" "cmn": "none"}', "expected ',' or '}' after \"feat\""),
])
def test_unusable_files_are_refused_by_name(tmp_path, body, words):
    p = tmp_path / "feat_params.json"
    p.write_text(body)
    with pytest.raises(ssw.SswError) as e:
        ssw.FeatConfig.read(str(p))
    assert words in str(e.value) and str(p) in str(e.value)
    with pytest.raises(ssw.SswError, match="Unknown CMN type"):
        ssw.FeatConfig.read(None, cmn="sometimes")


def test_shipped_models_are_plain(model):
    c = model.feat_config().as_dict()
    assert c["from_file"] and c["feat"] == "1s_c_d_dd" and c["cmn"] == "batch" and c["lda"] is None
    assert c["svspec"] == "0-12/13-25/26-38" and model.feat_plain()
    f = model.feat()
    assert (f.out_dim, f.raw_dim, f.window, f.stream_lens) == (39, 39, 3, [13, 13, 13])
    fr = ssw.Model(os.path.join(MODEL_ROOT, "fr-fr"), config=NONE)
    assert fr.feat_plain()
    fr.close()


def _model_dir(tmp_path, feat_params, transform=None):
    d = tmp_path / "m"
    d.mkdir()
    for n in ("mdef", "means", "variances", "sendump", "transition_matrices"):
        os.symlink(os.path.join(EN_US, n), d / n)
    if feat_params is not None:
        (d / "feat_params.json").write_text(json.dumps(feat_params))
    if transform is not None:
        shutil.copyfile(transform, d / "feature_transform")
    return str(d)


def test_feature_transform_beside_the_means_is_the_lda(tmp_path):
    d = _model_dir(tmp_path, {"cmn": "batch", "ldadim": 29}, FT.LDA_FILE)
    m = ssw.Model(d, config=NONE)
    c = m.feat_config().as_dict()
    assert c["lda"] == os.path.join(d, "feature_transform") and c["ldadim"] == 29
    assert not m.feat_plain()
    f = m.feat()
    assert (f.out_dim, f.raw_dim, f.stream_lens) == (29, 39, [29])
    m.close()


def test_no_feat_params_is_plain_and_a_bad_one_is_named(tmp_path):
    m = ssw.Model(_model_dir(tmp_path, None), config=NONE)
    assert m.feat_plain() and not m.feat_config().from_file
    assert m.feat_config().as_dict()["cmn"] == "live"        # the reference's default
    m.close()
    d = tmp_path / "b"
    d.mkdir()
    bad = _model_dir(d, {"cmn": "sometimes"})
    m = ssw.Model(bad, config=NONE)
    with pytest.raises(ssw.SswError, match='feat_params.json cannot be used: .*"sometimes"'):
        m.feat()
    m.close()


@pytest.mark.parametrize("name", sorted(FT.CASES))
def test_resolved_dimensions_are_the_references(model, fx, name):
    c = fx[name]
    f = model.feat(**_settings(c["settings"]))
    d = c["dims"]
    assert (f.out_dim, f.raw_dim, f.window, f.ceplen) == (d["width"], d["raw"], d["window"], d["ceplen"])
    r = FT.resolve(c["settings"])
    want = [len(r["lda"])] * len(r["sv"] or [0]) if r["lda"] is not None else \
        [len(v) for v in r["sv"]] if r["sv"] else r["streams"]
    assert f.stream_lens == want, name
    assert 1 <= f.tile_frames <= 64
    prior = FT.state_tuple(f.cmn_prior())
    n = r["ceplen"]
    assert prior[0][:n].tobytes() == r["prior"][0].tobytes() and prior[2] == r["prior"][2]
    assert prior[1][:n].tobytes() == r["prior"][1].tobytes() and not prior[0][n:].any()
    f.free()


def test_the_chain_of_comparisons_keeps_its_order(model):
    """prefixes, in the reference's order: 1s_c_d_dd before 1s_c_d before 1s_c; the cepwin types
    come last, so "1s_c..." never reaches them"""
    dims = lambda **kw: (lambda f: (f.raw_dim, f.window))(model.feat(**dict(PLAIN, **kw)))
    assert dims(feat="1s_c_d_dd_whatever") == (39, 3)
    assert dims(feat="1s_c_d_ld_dd.x") == (52, 4)
    assert dims(feat="1s_c_dx") == (26, 2) and dims(feat="cep_dcep2") == (26, 2)
    assert dims(feat="1s_cx") == (13, 0) and dims(feat="cepstra") == (13, 0)
    assert dims(feat="1s_3c!") == (91, 3) and dims(feat="1s_4c") == (117, 4)
    assert dims(feat="1s_c_d_dd", ceplen=20) == (60, 3) and dims(feat="1s_c", ceplen=0) == (13, 0)
    assert dims(feat="3,10") == (13, 0) and dims(feat="3,10:8") == (13 * 17, 8)
    assert dims(feat="13,") == (13, 0)               # as the reference scans it: %u reads "13,"


@pytest.mark.parametrize("kw,words", [
    (dict(feat="s2_4x", lda=FT.LDA_FILE), "LDA incompatible with multi-stream features (n_stream = 4)"),
    (dict(feat="s2_4x", svspec="0-11"), "Subvector specifications require single-stream features!"),
    (dict(feat="1s_c_d", lda=FT.LDA_FILE),
     "LDA matrix dimension 39 doesn't match feature stream size 26"),
    (dict(cmn="live", varnorm=True), "Variance normalization not implemented in live mode decode"),
    (dict(feat="s2_4x", ceplen=12), "s2_4x features require cepsize == 13"),
    (dict(feat="s3_1x39", ceplen=14), "s3_1x39 features require cepsize == 13"),
    (dict(feat="1s_12c_12d_3p_12dd", ceplen=14), "require cepsize == 13"),
    (dict(feat="12"), "Bad feature type argument"),
    (dict(feat="6,x"), "Bad feature type argument"),
    (dict(feat="6 7"), "Bad feature type argument"),
    (dict(feat="0,13"), "Bad feature type argument"),
    (dict(feat="mfcc"), "Bad feature type argument"),
    (dict(feat="13:9"), "a window of 9 frames (supported: 0..8)"),
    (dict(feat="1,1,1,1,1,1,1,1,5"), "9 streams (supported: at most 8)"),
    (dict(ceplen=65), "ceplen 65 (supported: 1..64)"),
    (dict(ceplen=-1), "ceplen -1 (supported: 1..64)"),
    (dict(svspec="0-12/x"), "Couldn't read int32 @pos 5"),
    (dict(svspec="0-"), "Couldn't read int32 @pos 2"),
    (dict(svspec="5-3"), "Bad subrange spec ending @pos 3"),
    (dict(svspec="0-3,2"), "Duplicate dimension ending @pos 5"),
    (dict(svspec="0-3;4"), "Bad delimiter @pos 3"),
    (dict(svspec="0-38/0"), "Total dimensionality of subvector specification 40 > feature dimensionality 39"),
    (dict(svspec="0-39"), "dimension 39 ending @pos 4 is beyond the 39 the stream has"),
    (dict(lda=FT.LDA_FILE, ldadim=12, svspec="0-12"),
     "Total dimensionality of subvector specification 13 > feature dimensionality 12"),
    (dict(lda=os.path.join(FT.DIR, "no_such_file")), "cannot open"),
    (dict(lda=FT.MFCC), "missing s3 signature"),
])
def test_refusals_by_their_words(model, kw, words):
    with pytest.raises(ssw.SswError) as e:
        model.feat(**dict(PLAIN, **kw))
    assert words in str(e.value), str(e.value)


def test_matrix_files_are_checked(model, tmp_path):
    FT.write_lda(str(tmp_path / "summed"), FT.read_lda(FT.LDA_FILE))   # (with a chksum0 header)
    assert model.feat(**dict(PLAIN, lda=str(tmp_path / "summed"))).out_dim == 36
    blob = open(tmp_path / "summed", "rb").read()
    p = tmp_path / "flipped"
    p.write_bytes(blob[:-8] + bytes([blob[-8] ^ 1]) + blob[-7:])
    with pytest.raises(ssw.SswError, match="checksum mismatch"):
        model.feat(**dict(PLAIN, lda=str(p)))
    p = tmp_path / "short"
    p.write_bytes(blob[:len(blob) // 2])
    with pytest.raises(ssw.SswError, match="truncated"):
        model.feat(**dict(PLAIN, lda=str(p)))
    wide = np.zeros((257, 39), np.float32)
    FT.write_lda(str(tmp_path / "rows257"), wide)
    with pytest.raises(ssw.SswError, match=r"257 rows of the LDA matrix are used \(supported: at most 256\)"):
        model.feat(**dict(PLAIN, lda=str(tmp_path / "rows257")))
    assert model.feat(**dict(PLAIN, lda=str(tmp_path / "rows257"), ldadim=256)).out_dim == 256
    assert FT.read_lda(FT.LDA_FILE).shape == (36, 39)


def test_compute_needs_a_device_and_the_models_ceplen(model):
    # (the buffers are never touched: every one of these is refused before a launch)
    with pytest.raises(ssw.SswError, match="SSW_DEVICE_NONE"):
        model.feat_batch_ex_device(1, 4, [0, 4], 1, model.feat(), None, ncep=13)
    with pytest.raises(ssw.SswError, match="12 cepstra per frame, but the configuration's ceplen is 13"):
        model.feat_batch_ex_device(1, 4, [0, 4], 1, model.feat(), None, ncep=12)
    with pytest.raises(ssw.SswError, match="utt_off must run from 0 to n_frames"):
        model.feat_batch_ex_device(1, 4, [0, 3, 2, 4], 1, model.feat(), None, ncep=13)


def test_c1_lda_model_is_exact(tmp_path):
    """the transform of model C1-lda: one entry +-2^e a row, at distinct columns, so every
    product and sum of the LDA is exact; means and variances follow it"""
    mat, perm, val = FT.c1_lda_matrix()
    assert mat.shape == (32, 39) and len(set(perm.tolist())) == 32
    assert (np.count_nonzero(mat, axis=1) == 1).all()
    assert set(np.abs(val).tolist()) <= {0.5, 1.0, 2.0}


# ---- the tile table ------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiles_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++") or shutil.which("clang++")
    assert cxx is not None, "no C++ compiler"
    tmp = tmp_path_factory.mktemp("feat_tiles")
    exe = str(tmp / "feat_tiles_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe,
                    os.path.join(ROOT, "tests", "harness", "feat_tiles_host.cpp")], check=True, cwd=str(tmp))
    return exe


def test_tile_table_under_sanitizers(tiles_exe):
    r = subprocess.run([tiles_exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.splitlines()[-1].startswith("ok: 400 "), \
        r.stdout[-2000:] + r.stderr[-2000:]


@pytest.mark.parametrize("tf,lens", [(64, [1, 2, 3, 7, 300, 0, 5, 63, 64, 65]), (10, [0, 0, 25, 10, 0]),
                                     (1, [3, 0, 2])])
def test_tile_table_is_the_restated_one(tiles_exe, tf, lens):
    r = subprocess.run([tiles_exe, str(tf)] + [str(n) for n in lens], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [tuple(int(x) for x in ln.split()[1:]) for ln in r.stdout.splitlines() if ln.startswith("T ")]
    assert got == FT.tiles(FT.offsets(lens), tf)


def test_make_feat_types_check_agrees_with_the_reference_build():
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_feat_types.py"),
                        "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr
