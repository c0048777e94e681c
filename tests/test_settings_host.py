"""logbase, varfloor, mixwfloor and tmatfloor away from their defaults, on the CPU.

Every loader reads the four settings and every kernel sees them through derived tables; here the
tables the library derives (device = SSW_DEVICE_NONE) are compared with the oracle's under each
setting of tests/settings_common.py, and both with what the reference library itself recorded
for the same settings (tests/golden/settings_results.json, written by
tests/golden/make_settings.py): the CRCs of det and the scaled variances, the count of floored
variances, and the rows of tests/golden/goforward.raw -- every frame by CRC, four frames whole.
The oracle restates the reference and had only been held against it at the default settings.

logbase selects code paths through the shape of the 8-bit log-add table: its largest entry T
decides whether the folded table of the senone kernel fits (255 + 96 + 3 T < 512, Hb <= 255) and
which kernel the ms scorer takes.  The table's properties by base (settings_common.LOGADD_ROWS)
are asserted, the fold helpers are fed every accepted table through the stand-alone harness of
tests/test_senone_fold_host.py, and the two scan bounds are replayed at the finest and the
coarsest base."""
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from tests import settings_common as SC
from tests.test_cabi_host import compare_with_oracle_tables
from tests.test_scan_bound import _mfma_bound_without_the_adder, scan_key_bound
from tests.test_senone_fold_host import _run, exe  # noqa: F401  (exe: the harness, a fixture)

NONE = ssw.SSW_DEVICE_NONE


@pytest.fixture(scope="module")
def fx():
    return SC.results()


@pytest.fixture(scope="module")
def fr_dir(orc_fr, tmp_path_factory):
    return SC.fr_mixw_dir(str(tmp_path_factory.mktemp("settings") / "fr-mixw"), orc_fr)


@pytest.fixture(scope="module")
def loaded(oracle_mod, fr_dir):
    """get(model, settings) -> (library model with tables only, oracle model); once per setting"""
    cache = {}

    def get(model, over):
        key = (model, tuple(sorted(over.items())))
        if key not in cache:
            cache[key] = (SC.load(model, over, NONE, fr_dir), SC.load_oracle(model, over, fr_dir))
        return cache[key]
    yield get
    for m, _ in cache.values():
        m.close()


@pytest.fixture(scope="module")
def oracle_rows(loaded):
    """get(case) -> the oracle's PTM rows of the recording under the case's settings"""
    cache = {}

    def get(case):
        if case not in cache:
            model, over = SC.SCORING[case]
            rows = loaded(model, over)[1].ptm_score_utt(SC.features(model))
            rows.setflags(write=False)
            cache[case] = rows
        return cache[case]
    return get


def test_make_settings_check_agrees_with_the_reference_build():
    if not reference.available():
        pytest.skip("no reference build in oracle/_ref/")
    r = subprocess.run([sys.executable, os.path.join(SC.ROOT, "tests", "golden", "make_settings.py"),
                        "--check"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout + r.stderr


# ---------------------------------------------------------------------------------------------
# the log-add table
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", sorted(SC.LOGADD_ROWS))
def test_logadd_table_by_base(oracle_mod, loaded, base):
    """the library's table is the oracle's, and has the row's properties: the largest entry, the
    last non-zero index, the reference's entry count (the oracle's: the library's API shows the
    first 256 entries only, and names the count in the ms scorer's refusal)"""
    t_max, last, entries = SC.LOGADD_ROWS[base]
    m, _ = loaded("en-us", {"logbase": base})
    lm = oracle_mod.Logmath(base, 10)
    want = lm.table()
    got = m.table("logadd8")
    assert lm.table_size == len(want) == entries
    assert len(got) == 256 and got.tolist() == want[:256].tolist()
    assert SC.logadd_properties(got) == (t_max, last)
    assert np.all(np.diff(got.astype(np.int64)) <= 0)
    if base == 1.001:
        assert got.tolist() == [1] + [0] * 255
    if base == 1.003:
        assert not got.any()


def test_logbase_too_small_is_refused_at_the_loader():
    with pytest.raises(ssw.SswError, match=r"log base 1\.00000\d too small for an 8-bit add table"):
        SC.load("en-us", {"logbase": SC.LOGBASE_REFUSED_AT_LOAD}, NONE)
    with pytest.raises(ssw.SswError, match="logbase must be > 1"):
        SC.load("en-us", {"logbase": 1.0}, NONE)


# ---------------------------------------------------------------------------------------------
# host loader tables
# ---------------------------------------------------------------------------------------------
def compare_loader_tables(m, o):
    """tests/test_cabi_host.py:test_host_loaders_match_oracle_tables's comparison, and the ms
    weights where the model has them"""
    compare_with_oracle_tables(m, o)
    assert bool(m.has_ms) == bool(o.has_ms_pdf)
    if m.has_ms:
        assert m.table("ms_pdf").tobytes() == o.ms_pdf.tobytes()


ALL_SETTINGS = sorted({(model, tuple(sorted(over.items())))
                       for model, over in list(SC.SCORING.values())
                       + [(mo, ov) for _, mo, ov in SC.FLOWS.values()]})


@pytest.mark.parametrize("model,over", ALL_SETTINGS,
                         ids=["%s-%s" % (m, "-".join("%s=%r" % kv for kv in o)) for m, o in ALL_SETTINGS])
def test_host_loaders_match_oracle_tables_under_the_setting(loaded, model, over):
    m, o = loaded(model, dict(over))
    compare_loader_tables(m, o)


def _table_crcs(m):
    """det[m][f][k] and var[m][f][k][j] as the driver walks them: the library's file order"""
    return SC.crc(m.table("det")), SC.crc(m.table("var"))


@pytest.mark.parametrize("case", sorted(SC.SCORING))
def test_det_and_var_are_the_references(loaded, fx, case):
    model, over = SC.SCORING[case]
    rec = fx["scoring"][case]
    m, o = loaded(model, over)
    assert _table_crcs(m) == (rec["det_crc"], rec["var_crc"])
    assert (SC.crc(o.det), SC.crc(o.var)) == (rec["det_crc"], rec["var_crc"])
    assert m.n_floored == o.n_floored == rec["n_floored"]
    assert rec["scorer"] == "ptm" and rec["frames"] == len(SC.features(model))


# ---------------------------------------------------------------------------------------------
# the settings do something
# ---------------------------------------------------------------------------------------------
def test_every_setting_changes_its_table(loaded):
    d_en = loaded("en-us", {})[0]
    for base in SC.LOGBASES_ACCEPTED:
        if base == SC.DEFAULTS["logbase"]:
            continue
        m = loaded("en-us", {"logbase": base})[0]
        assert m.table("logadd8").tolist() != d_en.table("logadd8").tolist(), base
        for tab in ("det", "var", "tp"):
            assert m.table(tab).tobytes() != d_en.table(tab).tobytes(), (base, tab)
        # (a sendump's bytes are the file's: the reference reads them whatever the base)
        assert m.table("ptm_mixw").tobytes() == d_en.table("ptm_mixw").tobytes()
    for vf in (1e-2, 1.0):
        m = loaded("en-us", {"varfloor": vf})[0]
        assert m.n_floored > d_en.n_floored and m.n_floored > 0, vf
        assert m.table("var").tobytes() != d_en.table("var").tobytes()
        assert m.table("det").tobytes() != d_en.table("det").tobytes()
    assert loaded("en-us", {"varfloor": 1.0})[0].n_floored > loaded("en-us", {"varfloor": 1e-2})[0].n_floored
    # tmatfloor: 0.3 raises entries of en-us's matrices.  1e-2 raises none: the floor touches the
    # non-zero probabilities only (and a zero on the two diagonals the reference names), and the
    # smallest non-zero probability of the file is above 1e-2 after the normalisation
    p = _nonzero_transition_probabilities(os.path.join(SC.EN_US, "transition_matrices"))
    assert 1e-2 < p.min() < 0.1 < 0.3
    assert loaded("en-us", {"tmatfloor": 0.3})[0].table("tp").tobytes() != d_en.table("tp").tobytes()
    assert loaded("en-us", {"tmatfloor": 0.1})[0].table("tp").tobytes() != d_en.table("tp").tobytes()
    assert loaded("en-us", {"tmatfloor": 0.1})[0].table("tp").tobytes() \
        != loaded("en-us", {"tmatfloor": 0.3})[0].table("tp").tobytes()
    assert loaded("en-us", {"tmatfloor": 1e-2})[0].table("tp").tobytes() == d_en.table("tp").tobytes()
    d_fr = loaded("fr-mixw", {})[0]
    for mf in (1e-3, 0.05):
        m = loaded("fr-mixw", {"mixwfloor": mf})[0]
        for tab in ("ptm_mixw", "ms_pdf"):
            n = int((m.table(tab) != d_fr.table(tab)).sum())
            assert n > 0, (mf, tab)


def _nonzero_transition_probabilities(path):
    """the non-zero entries of an s3 transition_matrices file, each row normalised to sum 1"""
    import struct
    with open(path, "rb") as fh:
        blob = fh.read()
    at = blob.index(b"endhdr\n") + len(b"endhdr\n")
    assert struct.unpack_from("<I", blob, at)[0] == 0x11223344
    n_tmat, n_src, n_dst, n = struct.unpack_from("<4i", blob, at + 4)
    tp = np.frombuffer(blob, "<f4", n, at + 20).reshape(n_tmat, n_src, n_dst).astype(np.float64)
    tp = tp / tp.sum(axis=2, keepdims=True)
    return tp[tp > 0]


def test_recorded_rows_differ_from_case_to_case(fx, oracle_rows, orc_en):
    """the reference's own rows: no two cases of a model recorded the same frames, and every
    logbase case differs from the rows at the default settings in every frame.  The varfloors
    touch few variances (108 and 176 of 209,664 against 98), of densities that hardly reach the
    top four on this recording: the rows at 1e-2 are the default's in all 278 frames and those at
    1.0 differ in one.  For the varfloors the pin is det, var and the floored count
    (test_det_and_var_are_the_references) and the frames of the next test; the recorded rows
    show that nothing else moved"""
    by_model = {}
    for case, rec in fx["scoring"].items():
        by_model.setdefault(rec["model"], []).append(tuple(rec["row_crc"]))
    for model, crcs in by_model.items():
        assert len(set(crcs)) == len(crcs), model
    default = SC.row_crcs(orc_en.ptm_score_utt(SC.features("en-us")))
    for case, rec in fx["scoring"].items():
        if rec["model"] == "en-us":
            n = sum(a != b for a, b in zip(default, rec["row_crc"]))
            print("%s: %d of %d frames differ from the default settings' rows" % (case, n, len(default)))
            if "logbase" in rec["settings"] and case.startswith("logbase"):
                assert n == len(default), case


@pytest.mark.parametrize("vf", [1e-2, 1.0])
def test_varfloor_moves_the_rows_near_floored_densities(loaded, orc_en, vf):
    """frames at the means of densities with a variance below the floor
    (settings_common.floored_density_features, the frames the GPU test scores): the oracle's rows
    under the floor are not the default's"""
    feats = SC.floored_density_features(vf, 48, 31)
    rows = loaded("en-us", {"varfloor": vf})[1].ptm_score_utt(feats)
    n = int((rows != orc_en.ptm_score_utt(feats)).any(axis=1).sum())
    print("varfloor %r: %d of %d rows differ from the default's" % (vf, n, len(feats)))
    assert n > len(feats) // 2


# ---------------------------------------------------------------------------------------------
# the oracle's rows are the reference's
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(SC.SCORING))
def test_oracle_rows_are_the_references(oracle_rows, fx, case):
    rec = fx["scoring"][case]
    rows = oracle_rows(case)
    assert len(rows) == rec["frames"]
    for t, want in rec["rows"].items():
        assert np.array_equal(rows[int(t)], np.array(want, np.int16)), t
    crcs = SC.row_crcs(rows)
    bad = [t for t in range(len(rows)) if crcs[t] != rec["row_crc"][t]]
    assert not bad, bad[:8]


def test_scores_tie_where_the_table_is_empty(oracle_rows):
    """logbase 1.003: log-add is a bare min and a score unit is 3 natural-log units; most senones
    of a frame share their score with another one"""
    rows = oracle_rows("logbase_1.003")
    distinct = np.array([len(np.unique(r)) for r in rows])
    assert distinct.max() < rows.shape[1] // 8, int(distinct.max())


def test_the_references_chains_read_past_256_entries_at_1_000015(oracle_mod, orc_en, tmp_path):
    """At 1.000015 the reference's add table has 317 entries, 256 to 316 all 1, and its log-add
    indexes the table unbounded (tied_mgau_common.h:100-117; the oracle likewise).  The kernels
    hold 256 entries and take 0 beyond, so the PTM and s2_semi scorers refuse such a base
    (tests/test_gpu_settings.py).  That the region is reached: the oracle's chains on the fold
    test's model (weights 0 and 255 side by side, clipped to 254) and frames, recomputed in numpy
    from its top-N block with the whole table (the oracle's rows) and with 256 entries (other
    rows)."""
    from tests import sc_common as S
    from tests.test_gpu_senone_fold import _extreme_features, _extreme_weights
    from tests.conftest import raw_means
    base = 1.000015
    sd = str(tmp_path / "sendump8")
    mixw = np.minimum(_extreme_weights(orc_en.n_feat, orc_en.n_density, orc_en.n_sen), 254)
    S.write_sendump8(sd, mixw)
    o = oracle_mod.Model(mdef=os.path.join(SC.EN_US, "mdef"), means=os.path.join(SC.EN_US, "means"),
                         vars=os.path.join(SC.EN_US, "variances"), sendump=sd,
                         tmat=os.path.join(SC.EN_US, "transition_matrices"), config={"logbase": base})
    full = o.logadd_table_8b.astype(np.int64)
    assert len(full) == 317 and (full[256:] == 1).all()
    # the library would serve this model but for the table's length: both of launch_senone's
    # conditions hold
    assert int((np.arange(255) + full[:255]).max()) <= 255 and 255 + 96 + 3 * int(full.max()) < 512
    feats = _extreme_features(raw_means(SC.EN_US))[40:72]      # the far frames and ordinary ones
    out, cw, sc = o.ptm_score_utt(feats, want_topn=True)
    w = mixw.astype(np.int64)
    sen2cb, sen = o.sen2cimap, np.arange(o.n_sen)
    n_beyond = n_rows_differ = 0
    for t in range(len(feats)):
        q = sc[t].reshape(-1, o.n_feat, 4)
        c = cw[t].reshape(-1, o.n_feat, 4)
        tot = {317: np.zeros(o.n_sen, np.int64), 256: np.zeros(o.n_sen, np.int64)}
        for size in tot:
            tab = np.concatenate([full[:size], np.zeros(2048, np.int64)])
            for f in range(o.n_feat):
                x = w[f, c[sen2cb, f, 0], sen] + q[sen2cb, f, 0]
                for k in range(1, 4):
                    y = w[f, c[sen2cb, f, k], sen] + q[sen2cb, f, k]
                    d = np.abs(x - y)
                    if size == 317:
                        n_beyond += int(((d >= 256) & (d < 317)).sum())
                    x = np.minimum(x, y) - tab[d]
                tot[size] += x
        assert np.array_equal((tot[317] - tot[317].min()).astype(np.int16), out[t]), t
        n_rows_differ += not np.array_equal(tot[317] - tot[317].min(), tot[256] - tot[256].min())
    print("%d chain steps read entries 256..316; %d of %d rows differ with 256 entries"
          % (n_beyond, n_rows_differ, len(feats)))
    assert n_beyond > 1000 and n_rows_differ > 0


# ---------------------------------------------------------------------------------------------
# the scan bounds at the finest and the coarsest base
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base", [1.000018, 1.003])
def test_scan_key_bound_under_logbase(oracle_mod, loaded, base):
    """tests/test_scan_bound.py:test_scan_key_bounds_the_reference_value with the records of
    another base: scores, and with them the keys, are 5.6 times larger or 30 times smaller in
    log units while the widening's constant term stays 1e-3.  At 1.000018 the host leaves 15,808
    of the 16,128 densities to the exact form (their bias would pass 4 score units), so only 320
    are scanned: this replay then says little about the vector-unit scan at that base, whose
    result there rests on the exact form (tests/test_gpu_settings.py, SSW_SCAN=fma)"""
    m, o = loaded("en-us", {"logbase": base})
    rng = np.random.default_rng(20240611)
    n_pairs, n_exact, worst_margin, worst_use = scan_key_bound(oracle_mod, m, o, "en-us %r" % base, rng)
    print("logbase %r: %d pairs, %d exact-form densities, min margin %.4g, share of the widening "
          "used %.3f" % (base, n_pairs, n_exact, worst_margin, worst_use))
    # (at 1.000018 the host leaves most densities to the exact form -- the printed count, kept in
    # profiles/settings_pins.json --: fewer pairs then, and the bound is asserted inside on each)
    # not vacuous: more than one scanned density per codebook-stream and input on average
    assert n_pairs > m.n_cb * m.n_feat * 770 and worst_use < 1.0


@pytest.mark.parametrize("base", [1.000018, 1.003])
def test_mfma_scan_bound_under_logbase(loaded, base):
    m, o = loaded("en-us", {"logbase": base})
    rng = np.random.default_rng(20261003)
    n_pairs, worst_margin, worst_use = _mfma_bound_without_the_adder(m, o.mean4(), rng, "en-us %r" % base)
    print("logbase %r: %d pairs, min margin %.4g, share of the widening used %.3f"
          % (base, n_pairs, worst_margin, worst_use))
    assert n_pairs > 2_500_000 and worst_use < 1.0


# ---------------------------------------------------------------------------------------------
# the fold helpers on every accepted table
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tabfiles(loaded, tmp_path_factory):
    d = tmp_path_factory.mktemp("tabs")
    out = {}
    for base in SC.LOGADD_ROWS:
        tab = loaded("en-us", {"logbase": base})[0].table("logadd8").astype(np.uint8)
        out[base] = (str(d / ("tab%r" % base)), tab)
        tab.tofile(out[base][0])
    return out


@pytest.mark.parametrize("base", SC.LOGBASES_ACCEPTED)
def test_fold_table_under_logbase(exe, tabfiles, tmp_path, base):  # noqa: F811
    """senone_fold_hb and senone_fold_table at wmax = 255: Hb <= 255, every entry a byte, and
    for every d = x - y from -(255 + 96 + 3 T) to wmax and every x a chain can hold
    x + H[d] - Hb = min(x, y) - tab[|d|]"""
    path, tab = tabfiles[base]
    t_max = SC.LOGADD_ROWS[base][0]
    t = np.zeros(4096, np.int64)
    t[:256] = tab
    hb_want = int((np.arange(256) + t[:256]).max())
    assert hb_want == 255
    assert 255 + 96 + 3 * t_max < 512, "launch_senone refuses this table"
    for size in (1024, 2048):
        out = str(tmp_path / ("h%d" % size))
        assert _run(exe, "table", path, 255, size, out)[-1] == "hb %d" % hb_want
        h = np.fromfile(out, np.uint8).astype(np.int64)
        assert len(h) == size
        low = 255 + (96 if size == 1024 else 640) + 3 * t_max
        if low >= size // 2:
            continue   # (the ms scorer keeps ms_senone_kernel at this base: no packed instance)
        d = np.arange(-low, 256)
        x = np.arange(-3 * t_max, low + 1)[:, None]
        y = x - d[None, :]
        assert np.array_equal(x + h[d + size // 2][None, :] - hb_want,
                              np.minimum(x, y) - t[np.abs(d)][None, :])


def test_tables_that_do_not_fold_are_reported(exe, tabfiles, tmp_path):  # noqa: F811
    """1.000015: Hb = 256 (tab[255] = 1); 1.00001 likewise: launch_senone refuses both"""
    for base in SC.LOGBASES_REFUSED_AT_SCORING:
        path, tab = tabfiles[base]
        out = str(tmp_path / ("h%r" % base))
        hb = int(_run(exe, "table", path, 255, 1024, out)[-1].split()[1])
        assert hb == int((np.arange(256) + tab.astype(np.int64)).max()) > 255
        assert not os.path.exists(out)
    # Hb follows the model's largest weight byte: at en-us's 158 (a mixture_weights file: at most
    # 159) the table of 1.000015 would fold, and 255 + 96 + 3 x 45 < 512.  The base is refused all
    # the same, for the table's 317 entries (test_the_references_chains_read_past_256_entries)
    path, tab = tabfiles[1.000015]
    out = str(tmp_path / "h158")
    hb = int((np.arange(160) + tab[:160].astype(np.int64)).max())
    assert 159 < hb < 255 and 255 + 96 + 3 * int(tab.max()) < 512
    assert _run(exe, "table", path, 159, 1024, out)[-1] == "hb %d" % hb
    assert os.path.getsize(out) == 1024
    assert _run(exe, "chains", path, 159, 0)[-1].startswith("ok: ")


# (no ms case where ms_takes_packed_kernel is false -- 255 + 640 + 6 T >= 1024 at 1.000018 and
# 1.00003 --: the ms scorer keeps ms_senone_kernel there, which has no folded table)
CHAIN_CASES = [(b, ms) for b in SC.LOGBASES_ACCEPTED if b != SC.DEFAULTS["logbase"] for ms in (0, 1)
               if not (ms and 255 + 640 + 6 * SC.LOGADD_ROWS[b][0] >= 1024)]


@pytest.mark.parametrize("base,ms", CHAIN_CASES,
                         ids=["%r-%s" % (b, "ms" if ms else "ptm") for b, ms in CHAIN_CASES])
def test_folded_chain_under_logbase(exe, tabfiles, base, ms):  # noqa: F811
    """the kernel's chain arithmetic against the reference's step with the table of another base:
    the extremes and two million random slot pairs, the look-up address inside the table"""
    lines = _run(exe, "chains", tabfiles[base][0], 255, ms)
    assert lines[-1].startswith("ok: "), lines[-3:]
    assert int(lines[-1].split()[1]) == 2000000 + 2048 * 2 * (11 if ms else 1)


# ---------------------------------------------------------------------------------------------
# the first-pass oracle follows the model's base
# ---------------------------------------------------------------------------------------------
def _first_pass_is_the_recognition(o, rec):
    """oracle/fsg_oracle.py on the oracle's rows of the recording against the reference's
    recognition of the text's chain grammar: the words with their frames, and a word's exit score
    the sum of ascr + lscr up to it"""
    from oracle import fsg_oracle as F
    olex = F.Lexicon(o, os.path.join(SC.EN_US, "dict.txt"), os.path.join(SC.EN_US, "noisedict.txt"))
    seg = F.first_pass(o, olex, SC.TEXT, o.ptm_score_utt(SC.features("en-us")))
    assert seg is not None
    assert " ".join(w for w, _, _, _ in seg if not w.startswith("<")) == rec["hyp"]
    want, total = [], 0
    for w, sf, ef, ascr, lscr, _ in rec["segments"]:
        total += ascr + lscr
        want.append((w, sf, ef, total))
    assert seg == want
    assert seg[-1][3] == rec["score"]
    return seg


def test_first_pass_oracle_at_logbase_1_0003(loaded, fx):
    """beams, penalties and filler probabilities are logs in the model's base: with 1.0001's on
    rows of 1.0003 the search is another one"""
    import json
    o = loaded("en-us", {"logbase": 1.0003})[1]
    assert o.logbase == 1.0003
    seg = _first_pass_is_the_recognition(o, fx["flows"]["rec_chain_logbase_1.0003"])
    # the first pass of the reference's text alignment is the same search
    words = json.loads(fx["flows"]["align_logbase_1.0003"]["json"])["w"]
    assert [(w["t"], round(w["b"] * 100), round(w["d"] * 100)) for w in words] \
        == [(w, sf, ef - sf + 1) for w, sf, ef, _ in seg]


def test_first_pass_oracle_at_the_default_base(orc_en, fx):
    """at 1.0001 it gives what it gave while the base was a literal: the reference's record"""
    assert orc_en.logbase == 1.0001
    _first_pass_is_the_recognition(orc_en, fx["flows"]["rec_chain_default"])
    assert fx["flows"]["rec_chain_default"]["score"] != fx["flows"]["rec_chain_logbase_1.0003"]["score"]
