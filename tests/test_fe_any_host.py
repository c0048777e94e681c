"""The front end under any settings fe_init accepts, host side (no GPU): what ssw_fe_create and
ssw_fe_batch_any refuse and in which words, the row width of every mode, the warp strings and
ssw_model_fe_plain of a model directory, frame counts, empty batches, the proof that decides how
remove_dc sums a frame, the host table builder under AddressSanitizer + UBSan in a program of its
own, and (where build() made the reference library) that the committed fixtures are what the
reference makes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from tests import fe_any_common as A
from tests.conftest import MODEL_ROOT, ROOT

CSRC = os.path.join(ROOT, "soundswallower_amd", "csrc")


@pytest.fixture(scope="module")
def cpu_en():
    _lib.build()
    return ssw.Model(os.path.join(MODEL_ROOT, "en-us"), config={"device": -2})


def _model_with_params(tmp_path, params):
    src = os.path.join(MODEL_ROOT, "en-us")
    for f in os.listdir(src):
        if f != "feat_params.json":
            os.symlink(os.path.join(src, f), tmp_path / f)
    (tmp_path / "feat_params.json").write_text(json.dumps(params))
    return ssw.Model(str(tmp_path), config={"device": -2})


def _en_us(**over):
    p = json.load(open(os.path.join(MODEL_ROOT, "en-us", "feat_params.json")))
    p.update(over)
    return p


@pytest.mark.parametrize("cfg,warp_type,warp_params,words", [
    ({"dither": True}, None, None, "dither is not supported: its random stream belongs to a "
                                   "process's lifetime"),
    ({}, "bilinear", "1.1", "Unimplemented warping function bilinear"),
    ({"warp": 1}, None, None, "warp is set but no warp_params are given"),
    ({"warp": 1}, "affine", "", "warp is set but no warp_params are given"),
    ({"ncep": 0}, None, None, r"ncep must be 1\.\.64 and nfilt 1\.\.64 \(got 0, 20\)"),
    ({"ncep": 65}, None, None, r"ncep must be 1\.\.64 and nfilt 1\.\.64 \(got 65, 20\)"),
    ({"nfilt": 0}, None, None, r"ncep must be 1\.\.64 and nfilt 1\.\.64 \(got 13, 0\)"),
    ({"nfilt": 65}, None, None, r"ncep must be 1\.\.64 and nfilt 1\.\.64 \(got 13, 65\)"),
    ({"transform": 7}, None, None, "unknown transform 7"),
    ({"alpha": float("inf")}, None, None, "not a finite float32"),
    ({"alpha": 1e300}, None, None, "not a finite float32"),
    ({"lifter": -1}, None, None, "lifter must be >= 0"),
    ({"lowerf": 4000.0}, None, None, "0 <= lowerf < upperf"),
    ({}, "affine", "1 " * 200, "warp_params is longer than 255 characters"),
])
def test_create_refuses_by_name(cpu_en, cfg, warp_type, warp_params, words):
    with pytest.raises(ssw.SswError, match=words):
        cpu_en.fe(cfg, warp_type, warp_params)


def test_input_endian_other_than_the_hosts_is_refused(tmp_path):
    other = "big" if sys.byteorder == "little" else "little"
    m = _model_with_params(tmp_path, _en_us(input_endian=other))
    assert not m.fe_plain()
    with pytest.raises(ssw.SswError, match=f"input_endian {other} is not the host's"):
        m.fe()
    # the older entry points never read the key: they go on as before
    assert m.fe_batch(np.zeros(0, np.int16))[0].shape == (0, 13)


@pytest.mark.parametrize("cfg,rate,words", [
    # the bank's outer edges: one filter width below lowerf, above upperf
    ({"doublebw": True, "lowerf": 20.0}, 16000, "doublebw: the outer filter edges .* are outside"),
    ({"doublebw": True, "lowerf": 130.0, "upperf": 7900.0}, 16000, "doublebw: the outer filter edges"),
    ({"round_filters": False, "lowerf": 100.0, "upperf": 130.0, "nfilt": 40}, 16000,
     "covers no DFT point"),
    ({"lowerf": 100.0, "upperf": 200.0, "nfilt": 40}, 16000, "narrower than one DFT point"),
    ({"remove_dc": True}, 44100.5, "whole number"),
    ({"remove_dc": True, "upperf": 6000.0}, 8000, "upperf 6000 is above samprate / 2"),
])
def test_the_first_rate_where_it_shows_refuses(cpu_en, cfg, rate, words):
    """settings that resolve, refused where a rate's tables are built -- before any device call:
    the model has no device, and the batch no samples"""
    fe = cpu_en.fe(cfg)
    with pytest.raises(ssw.SswError, match=words):
        cpu_en.fe_batch_any(np.zeros(0, np.int16), rate, fe)
    fe.free()


def test_the_older_entry_points_refuse_as_before(cpu_en):
    for cfg, words in (({"remove_dc": True}, "remove_dc is not supported"),
                       ({"transform": "htk"}, "transform = htk is not supported"),
                       ({"ncep": 12}, "only ncep 13 and alpha 0.97"),
                       ({"round_filters": False}, "only unit_area = yes and round_filters = yes")):
        with pytest.raises(ssw.SswError, match=words):
            cpu_en.fe_batch_rates(np.zeros(0, np.int16), 16000, cfg=cfg)


@pytest.mark.parametrize("cfg,width", [
    ({}, 13), ({"ncep": 1}, 1), ({"ncep": 26}, 26), ({"ncep": 64}, 64),
    ({"transform": "htk"}, 13), ({"logspec": True}, 20), ({"smoothspec": True}, 20),
    ({"smoothspec": True, "logspec": True, "ncep": 5}, 20),
    (dict(A.WIDE, logspec=True), 40), ({"logspec": True, "ncep": 30}, 20)])
def test_out_dim(cpu_en, cfg, width):
    fe = cpu_en.fe(cfg)
    assert fe.out_dim == width
    rows, fo = cpu_en.fe_batch_any(np.zeros(0, np.int16), 16000, fe)     # no device needed
    assert rows.shape == (0, width) and list(fo) == [0, 0]
    fe.free()


def test_warp_strings_and_fe_plain_of_a_model_directory(tmp_path, cpu_en):
    assert cpu_en.fe_plain() and cpu_en.fe_warp() == ("inverse_linear", "")
    cases = (
        ({}, True, ("inverse_linear", "")),
        ({"warp_params": ""}, True, ("inverse_linear", "")),           # reads as no warping
        ({"warp_params": None}, True, ("inverse_linear", "")),
        ({"warp_type": "affine"}, True, ("affine", "")),               # a type alone warps nothing
        ({"warp_type": "piecewise_linear", "warp_params": "0.9 3000"}, False,
         ("piecewise_linear", "0.9 3000")),
        ({"warp_params": "1.1"}, False, ("inverse_linear", "1.1")),
        ({"remove_dc": True}, False, ("inverse_linear", "")),
        ({"round_filters": False}, False, ("inverse_linear", "")),
        ({"alpha": 0.95}, False, ("inverse_linear", "")),
        ({"ncep": 12, "ceplen": 12}, False, ("inverse_linear", "")),
    )
    for k, (over, plain, warp) in enumerate(cases):
        d = tmp_path / f"m{k}"
        d.mkdir()
        m = _model_with_params(d, _en_us(**over))
        assert m.fe_plain() == plain, over
        assert m.fe_warp() == warp, over
        assert m.fe_config().warp == int(bool(warp[1])), over
        fe = m.fe()                                     # the model's settings, its strings with them
        assert fe.out_dim == over.get("ncep", 13)
        fe.free()
        m.close()


def test_warp_parameters_belong_to_the_fe(cpu_en):
    """two configurations with different warps side by side: the first keeps its own (the
    reference keeps one set per process)"""
    a = cpu_en.fe({}, "affine", "1.05 20 and more that is ignored")
    b = cpu_en.fe({}, "piecewise", "0.9")              # the short name; F = 0: 0.85 samprate
    c = cpu_en.fe({}, "inverse_linear", "0")           # slope 0: no warping
    for fe in (a, b, c, a):
        rows, fo = cpu_en.fe_batch_any(np.zeros(0, np.int16), 16000, fe)
        assert rows.shape == (0, 13)
    for fe in (a, b, c):
        fe.free()


def test_frame_counts(cpu_en):
    gold = np.load(A.MFCC_NPZ)
    for fx in A.FIXTURES:
        name, rate, cfg, _, _ = fx
        s, wt, wp = A.settings(cfg)
        fe = cpu_en.fe(s, wt, wp)
        n = len(A.fixture_pcm(fx))
        want = gold["cep/" + name]
        assert int(fe.frames(n, rate)) == len(want), name
        assert fe.out_dim == want.shape[1], name
        assert int(ssw.fe_frame_counts_at([n], rate, wlen=s.get("wlen", 0.025625))[0]) == len(want)
        fe.free()
    fe = cpu_en.fe({"remove_dc": True})
    assert list(fe.frames([0, 1, 409, 410, 411, 569, 570, 571])) == [0, 1, 1, 2, 2, 2, 3, 3]
    assert list(fe.frames([0, 1130, 205], [8000, 44100, 8000])) == [0, 2, 2]
    with pytest.raises(ssw.SswError, match="whole number"):
        fe.frames([10], 0.5)
    fe.free()


def test_empty_batches_need_no_device(cpu_en):
    fe = cpu_en.fe({"remove_dc": True, "transform": "htk"})
    rows, fo = cpu_en.fe_batch_any([np.zeros(0, np.int16)] * 3, [8000, 16000, 44100], fe)
    assert rows.shape == (0, 13) and list(fo) == [0, 0, 0, 0]
    rows, fo = cpu_en.fe_batch_any([np.zeros(0, np.float32)], 16000, fe)
    assert rows.shape == (0, 13) and list(fo) == [0, 0]
    with pytest.raises(ssw.SswError, match="device"):       # samples need one
        cpu_en.fe_batch_any(np.zeros(500, np.int16), 16000, fe)
    fe.free()


@pytest.mark.skipif(not reference.available(), reason="no reference build in oracle/_ref/")
def test_committed_fixtures_are_what_the_reference_makes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_fe_any.py"),
                        "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr


def test_fixture_files_are_small():
    from tests import fe_rates_common as R
    assert os.path.getsize(A.MFCC_NPZ) < os.path.getsize(R.MFCC_NPZ)
    gold = np.load(A.MFCC_NPZ)
    assert sorted(gold.files) == sorted("cep/" + f[0] for f in A.FIXTURES)
    plain = np.load(os.path.join(A.GOLD, "goforward_mfcc.npy")).astype(np.float32)[:149]
    for f in A.FIXTURES:
        rows = gold["cep/" + f[0]]
        assert np.isfinite(rows).all(), f[0]
        if rows.shape == plain.shape and f[1] == 16000:
            assert rows.tobytes() != plain.tobytes(), f[0]       # the setting changes the rows


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("fe_any_asan") / "fe_any_host_main")
    cmd = ["gcc", "-O1", "-g", "-std=gnu99", "-Wall", "-fsanitize=address,undefined",
           "-fno-omit-frame-pointer", "-ffp-contract=off", "-I" + os.path.join(ROOT, "include"),
           "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "harness", "fe_any_host_main.c"),
           os.path.join(CSRC, "ssw_model.c"), "-lm", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


def test_host_tables_are_clean_under_asan_ubsan(program, tmp_path):
    """every fixture's settings through the host path that ssw_fe_batch_any takes, in a program
    of its own; how each remove_dc fixture's frames are summed is what the fixture is there for"""
    args, names = [], []
    for k, (name, rate, cfg, _, kind) in enumerate(A.FIXTURES):
        path = str(tmp_path / f"{name}.json")
        with open(path, "w") as f:
            json.dump(_en_us(**cfg), f)
        args += ["ok", path, str(rate), str(int(A.KINDS[kind][0] == "f32"))]
        names.append(name)
    refused = (({"dither": True}, "dither is not supported"),
               ({"warp_type": "bilinear", "warp_params": "1"}, "Unimplemented warping function"),
               ({"doublebw": True, "lowerf": 20.0}, "doublebw: the outer filter edges"),
               ({"lowerf": 100.0, "upperf": 200.0, "nfilt": 40}, "narrower than one DFT point"),
               ({"ncep": 65}, "ncep must be 1..64"))
    for k, (cfg, words) in enumerate(refused):
        path = str(tmp_path / f"refused{k}.json")
        with open(path, "w") as f:
            json.dump(_en_us(**cfg), f)
        args += ["bad", path, "16000", words]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")
    r = subprocess.run([program] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr
    lines = r.stdout.splitlines()
    assert lines[-1] == "ok %d built, %d refused" % (len(names), len(refused)), r.stdout
    dc = {n: int(ln.split()[-1]) for n, ln in zip(names, lines)}
    plain = {n: int(ln.split()[-4]) for n, ln in zip(names, lines)}
    assert not any(plain.values())                     # none is a setting the older entries take
    assert dc["alpha095"] == 0 and dc["remove_dc"] == 1 and dc["combo8000"] == 1
    assert dc["dc_offset900"] == 1 and dc["dc_len1"] == 1
    assert dc["dc_192000_alpha0001"] == 2              # int16, alpha on too fine a grid
    assert dc["dc_f32_third"] == 2 and dc["dc_f32_exact"] == 2   # float32: always in order


def test_the_exactness_proof_on_the_cases_checked_by_hand(program, tmp_path):
    """int16 samples: every order of summing agrees at alpha 0.97 and 0.95 up to 8192 samples and
    at 0.3 for 4920; at 0.001 orders disagree (the ordered sum is taken); and the bound is not
    loose by much: a frame summed in any order is in fact exact"""
    rng = np.random.default_rng(3)
    for alpha, size in ((0.97, 410), (0.97, 8192), (0.95, 8192), (0.3, 4920)):
        a = float(np.float32(alpha))
        x = rng.integers(-32768, 32768, size + 1).astype(np.float64)
        frame = x[1:] - x[:-1] * a
        fwd = 0.0
        for v in frame:
            fwd += v
        assert fwd == float(np.sum(frame[::-1])) == float(np.sum(frame)), (alpha, size)
    cases = ((0.97, 16000, 1), (0.95, 192000, 1), (0.3, 192000, 1), (0.001, 192000, 2),
             (0.0, 192000, 1), (0.001, 8000, 2), (0.5, 16000, 1), (1e-30, 16000, 2))
    args = []
    for k, (alpha, rate, _) in enumerate(cases):
        path = str(tmp_path / f"a{k}.json")
        with open(path, "w") as f:
            json.dump(_en_us(remove_dc=True, alpha=alpha), f)
        args += ["ok", path, str(rate), "0"]
    r = subprocess.run([program] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    got = [int(ln.split()[-1]) for ln in r.stdout.splitlines()[:-1]]
    assert got == [c[2] for c in cases]
