"""MLLR speaker adaptation on the host (ssw_mllr_*, ssw_model_apply_mllr on SSW_DEVICE_NONE
models): the parser, every refusal by its message, what identity, re-applying and clearing do to
the host tables, the generation counter, and a numpy restatement of gauden_mllr_transform +
gauden_dist_precompute (tests/mllr_common.restate) against the library's mean, var and det tables
for all five models and all transforms."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from soundswallower_amd.api import _TABLES
from tests import mllr_common as M

NONE = ssw.SSW_DEVICE_NONE


@pytest.fixture(scope="module")
def kwargs(tmp_path_factory):
    from soundswallower_amd import _lib
    _lib.build()
    return M.model_kwargs(str(tmp_path_factory.mktemp("mllr_models")))


@pytest.fixture(scope="module")
def en(kwargs):
    return M.load(kwargs["en-us"], NONE)


def tables(m):
    return {n: m.table(n).tobytes() for n in _TABLES}


def read(name, layout="3x13"):
    return ssw.Mllr.read(M.transform_path(name, layout))


# ---- the parser ------------------------------------------------------------------------------
def test_parser_reads_a_hand_written_file(tmp_path):
    p = tmp_path / "t.mllr"
    p.write_text("2\n2\n2\n1 2\n3 4\n5 6\n7 8\n-1 -2\n-3 -4\n-5 -6\n-7 -8\n"
                 "1\n0.5\n1e-3\n2\n9\n10\n11\n")
    t = ssw.Mllr.read(str(p))
    assert t.n_class == 2 and t.veclen == [2, 1]
    A, b, h = t.arrays(0)
    assert A[0].tolist() == [[1, 2], [3, 4]] and b[0].tolist() == [5, 6] and h[0].tolist() == [7, 8]
    assert A[1].tolist() == [[0.5]] and b[1][0] == np.float32(1e-3) and h[1].tolist() == [2]
    A, b, h = t.arrays(1)
    assert A[0].tolist() == [[-1, -2], [-3, -4]] and b[0].tolist() == [-5, -6]
    assert h[0].tolist() == [-7, -8] and (A[1][0, 0], b[1][0], h[1][0]) == (9, 10, 11)


def test_committed_files_are_the_generated_transforms():
    for layout in M.LAYOUTS:
        for name in M.TRANSFORMS:
            classes = M.transform_arrays(name, layout, M.results()["scale"])
            t = read(name, layout)
            assert t.n_class == len(classes) and t.veclen == list(M.LAYOUTS[layout])
            for k, want in enumerate(classes):
                for got_s, want_s in zip(t.arrays(k), want):
                    for g, w in zip(got_s, want_s):
                        assert g.tobytes() == w.tobytes(), (name, layout, k)


@pytest.mark.parametrize("text, words", [
    ("", "number of MLLR classes"),
    ("0\n3\n", "0 MLLR classes, at least one"),
    ("-1\n", "-1 MLLR classes"),
    ("1\n", "short file: cannot read the number of feature streams"),
    ("1\n9\n", "9 feature streams"),
    ("1\n1\n", "short file: cannot read the length of stream 0"),
    ("1\n1\n0\n", "stream 0 has 0 dimensions"),
    ("1\n1\n2\n1 0 0\n", "short file: cannot read the MLLR rotation"),
    ("1\n1\n2\n1 0 0 1\n0\n", "short file: cannot read the MLLR bias"),
    ("1\n1\n2\n1 0 0 1\n0 0\n1\n", "short file: cannot read the MLLR variance scale"),
    ("1\n1\n2\n1 0 x 1\n0 0\n1 1\n", "short file: cannot read the MLLR rotation"),
])
def test_parser_refusals(tmp_path, text, words):
    p = tmp_path / "bad.mllr"
    p.write_text(text)
    with pytest.raises(ssw.SswError, match=words):
        ssw.Mllr.read(str(p))


def test_unreadable_file(tmp_path):
    with pytest.raises(ssw.SswError, match="cannot open the MLLR file"):
        ssw.Mllr.read(str(tmp_path / "none.mllr"))
    with pytest.raises(ssw.SswError, match="cannot open the MLLR file"):
        ssw.Model(ssw.model_dir("en-us"), config={"device": NONE}, mllr=str(tmp_path / "none.mllr"))


# ---- refusals of apply: the model does not move -------------------------------------------------
def test_apply_refusals_leave_the_model_alone(en):
    en.apply_mllr(None)
    before, gen = tables(en), en.mllr_generation
    eye, zero, one = np.eye(13, dtype=np.float32), np.zeros(13, np.float32), np.ones(13, np.float32)
    nan = eye.copy()
    nan[3, 4] = np.nan
    inf_b, inf_h = zero.copy(), one.copy()
    inf_b[0], inf_h[12] = np.inf, -np.inf
    cases = [
        (ssw.Mllr(A=[eye] * 2, b=[zero] * 2, h=[one] * 2), "2 feature streams, the model has 3"),
        (ssw.Mllr(A=[eye, eye, np.eye(12)], b=[zero, zero, zero[:12]], h=[one, one, one[:12]]),
         "stream 2 has 12 dimensions, the model's has 13"),
        (read("mild", "1x39"), "1 feature streams, the model has 3"),
        (ssw.Mllr(A=[eye, nan, eye], b=[zero] * 3, h=[one] * 3), "non-finite number in row 3 of stream 1"),
        (ssw.Mllr(A=[eye] * 3, b=[inf_b, zero, zero], h=[one] * 3), "non-finite number in row 0 of stream 0"),
        (ssw.Mllr(A=[eye] * 3, b=[zero] * 3, h=[one, one, inf_h]), "non-finite number in row 12 of stream 2"),
    ]
    for t, words in cases:
        with pytest.raises(ssw.SswError, match=words):
            en.apply_mllr(t)
        assert tables(en) == before and en.mllr_generation == gen
    # n_class < 1 cannot be made through the constructors: a struct whose count says so
    t = read("mild")
    t._struct().n_class = 0
    with pytest.raises(ssw.SswError, match="0 classes, at least one"):
        en.apply_mllr(t)
    t._struct().n_class = 1
    assert tables(en) == before and en.mllr_generation == gen
    with pytest.raises(ssw.SswError, match="at least one"):
        ssw.Mllr._create_raw(0, [13], [eye], [zero], [one])


# ---- what apply does to the tables ---------------------------------------------------------------
def test_identity_clear_reapply_and_generation(kwargs):
    for model, (layout, _) in M.MODELS.items():
        m = M.load(kwargs[model], NONE)
        loaded = tables(m)
        assert m.mllr_generation == 0
        m.apply_mllr(read("identity", layout))
        assert tables(m) == loaded, model  # every table ssw_model_table names, byte for byte
        assert m.mllr_generation == 1
        if model in ("en-us", "C1"):
            a, b = read("mild", layout), read("var", layout)
            m.apply_mllr(a)
            ta = tables(m)
            assert ta != loaded and m.mllr_generation == 2
            m.apply_mllr(a)
            assert tables(m) == ta, "applying twice is not applying once"
            m.apply_mllr(b)
            tb = tables(m)
            assert tb != ta
            m.apply_mllr(a)
            assert tables(m) == ta, "A, B, A does not give A's tables"
            m.apply_mllr(read("two_class", layout))
            assert tables(m) == ta, "class 1 was used"
            m.apply_mllr(None)
            assert tables(m) == loaded and m.mllr_generation == 7
        m.close()


def test_model_mllr_keyword(kwargs):
    m = ssw.Model(ssw.model_dir("en-us"), config={"device": NONE},
                  mllr=M.transform_path("var", "3x13"))
    assert m.mllr_generation == 1
    assert tables(m)["rec"] != tables(M.load(kwargs["en-us"], NONE))["rec"]
    en2 = M.load(kwargs["en-us"], NONE)
    en2.apply_mllr(read("var"))
    assert tables(m) == tables(en2)


def test_floor_transform_counts_the_floored_variances(en, kwargs):
    """h = 1e-6 sends every variance below 100 under varfloor = 1e-4 (en-us has larger ones too):
    n_floored follows the adapted variances, and goes back with them"""
    en.apply_mllr(None)
    loaded = en.n_floored
    _, var0 = S_read(kwargs["en-us"])
    scaled = (var0 * np.float32(1e-6)).astype(np.float32)
    en.apply_mllr(read("floor"))
    assert en.n_floored == int(np.count_nonzero(scaled < np.float32(1e-4))) > var0.size // 2
    en.apply_mllr(None)
    assert en.n_floored == loaded == int(np.count_nonzero(var0 < np.float32(1e-4)))


# ---- the arithmetic -----------------------------------------------------------------------------
def test_restatement_gives_the_library_tables(kwargs):
    for model, (layout, _) in M.MODELS.items():
        m = M.load(kwargs[model], NONE)
        mean0, var0 = S_read(kwargs[model])
        for name in M.TRANSFORMS:
            t = read(name, layout)
            m.apply_mllr(t)
            mean, var, det = M.restate(mean0, var0, m.veclen, m.n_cb, m.n_density, *t.arrays(0))
            assert m.table("mean").tobytes() == mean.tobytes(), (model, name)
            assert m.table("var").tobytes() == var.tobytes(), (model, name)
            assert m.table("det").tobytes() == det.tobytes(), (model, name)
        m.close()


def S_read(kw):
    """the means and variances of a model's files, flat float32 in file order"""
    from tests import sc_common as S
    d = kw.get("path")
    out = []
    for key, name in (("means", "means"), ("variances", "variances")):
        path = kw[key] if d is None else os.path.join(d, name)
        n_cb, _, streams = S.read_gauss(path)
        out.append(np.concatenate([s.reshape(n_cb, -1) for s in streams], axis=1).reshape(-1))
    return out
