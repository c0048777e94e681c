#!/usr/bin/env python3
"""Writes the fixtures of the MLLR speaker-adaptation tests:

    tests/golden/mllr/<transform>_<layout>.mllr
        the transforms of tests/mllr_common, from soundswallower_amd.synth.lcg_uniform, in the
        reference's text format
    tests/golden/mllr_results.json, tests/golden/mllr/rows.npz (the whole rows, int16),
    tests/golden/mllr/goforward_fr_feat.npy (the feature rows the reference scored with fr-fr)
        the reference library, built by build() into oracle/_ref/, through
        tests/harness/mllr_driver.c over tests/golden/goforward.raw:
          scoring.<model>/<transform>  scorer, det_crc, var_crc, frames, row_crc [frames], rows
                                       {frame: [n_sen]} for frames 0, 1, 2 and the last;
                                       compallsen = yes; models en-us (ptm), fr-fr (ms, with the
                                       mixture weights of mllr_common.fr_mixw), cb41 (s2_semi),
                                       C3 and C1 of tests/cont_common
          scoring.en-us_ds2/mild       the same with ds = 2 (the chain kernel's row set)
          rec.<model>/<transform>/<grammar>, align.<model>/<transform>
                                       en-us and C3 under mild and var, compallsen = yes
          rec_default.<grammar>, align_default
                                       en-us under mild in the default configuration
          scale                        what SCALE_A and SCALE_B were multiplied by (1: as written)
    Every case is run both ways -- mllr = FILE at decoder_init, and mllr_read +
    decoder_apply_mllr on a running decoder -- and the two must print the same.  Under every
    non-identity transform the reference must still find a hypothesis and an alignment; if not,
    the scales are halved and `scale` says so.

    python tests/golden/make_mllr.py           # rewrite the fixtures
    python tests/golden/make_mllr.py --check   # rewrite nothing; exit 1 and name what would change
"""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import mllr_common as M  # noqa: E402
from tests import sc_common as S  # noqa: E402
from tests.golden.make_sc import parse_rec, parse_scoring, run  # noqa: E402

SPOKEN = ("mild", "var")


def build_driver(tmp):
    exe = os.path.join(tmp, "mllr_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "mllr_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def both_ways(exe, mode, hmm, mllr, *rest):
    """the driver's output with the transform given both ways; they must agree"""
    a = run(exe, mode, hmm, "config", mllr, *rest)
    b = run(exe, mode, hmm, "apply", mllr, *rest)
    assert a == b, "%s %s %s: mllr = FILE and decoder_apply_mllr disagree" % (mode, hmm, mllr)
    return a


def transform_files(tmp, scale):
    out = {}
    for layout in M.LAYOUTS:
        for name in M.TRANSFORMS:
            p = os.path.join(tmp, os.path.basename(M.transform_path(name, layout)))
            with open(p, "w", encoding="ascii") as fh:
                fh.write(M.transform_text(M.transform_arrays(name, layout, scale)))
            out[name, layout] = p
    return out


def model_dirs(tmp):
    """name -> (directory for the reference's hmm key, MIXW argument)"""
    kw = M.model_kwargs(tmp)
    return {"en-us": (S.EN_US, "-"), "fr-fr": (M.FR_FR, kw["fr-fr"]["mixw"]),
            "cb41": (os.path.join(tmp, "cb41"), "-"), "C3": (os.path.join(tmp, "C3"), "-"),
            "C1": (os.path.join(tmp, "C1"), "-")}


def generate(tmp, scale):
    """(results, fr-fr's feature rows), or None when a non-identity transform at this scale
    leaves the reference without a hypothesis or an alignment"""
    exe = build_driver(tmp)
    files = transform_files(tmp, scale)
    dirs = model_dirs(tmp)
    fsg = lambda g: os.path.join(M.GOLD, "fsg", g + ".fsg")
    got = {"scoring": {}, "rec": {}, "align": {}, "rec_default": {}, "align_default": None,
           "scale": scale}

    def spoken(hmm, mllr, compallsen):
        recs = {g: parse_rec(both_ways(exe, "rec", hmm, mllr, compallsen, fsg(g), M.PCM))
                for g in M.GRAMMARS}
        a = parse_rec(both_ways(exe, "align", hmm, mllr, compallsen, M.PCM))
        ok = all(r["hyp"] for r in recs.values()) and a["json"] and '"w":[]' not in a["json"]
        return recs, {"scorer": a["scorer"], "json": a["json"]}, ok

    # the condition first: it decides the scale
    for model in ("en-us", "C3"):
        for name in SPOKEN:
            recs, al, ok = spoken(dirs[model][0], files[name, M.MODELS[model][0]], "yes")
            if not ok:
                return None
            for g, r in recs.items():
                got["rec"]["%s/%s/%s" % (model, name, g)] = r
            got["align"]["%s/%s" % (model, name)] = al
    recs, al, ok = spoken(dirs["en-us"][0], files["mild", "3x13"], "default")
    if not ok:
        return None
    got["rec_default"], got["align_default"] = recs, al

    featout = os.path.join(tmp, "feat.f32")
    fr_feat = None
    for model, (layout, scorer) in M.MODELS.items():
        hmm, mixw = dirs[model]
        for name in M.TRANSFORMS:
            rec = parse_scoring(both_ways(exe, "score", hmm, files[name, layout], mixw, 1, M.PCM,
                                          featout))
            assert rec["scorer"] == scorer, (model, rec["scorer"])
            feats = np.fromfile(featout, "<f4").reshape(-1, 39)
            if model == "fr-fr":
                fr_feat = feats
            else:
                assert np.array_equal(feats, np.load(S.FEAT_A)), \
                    "the reference's feature rows are not tests/golden/sc/goforward_feat.npy"
            got["scoring"]["%s/%s" % (model, name)] = rec
        # the untransformed model through the same driver: identity must give its rows
        base = parse_scoring(run(exe, "score", hmm, "none", "-", mixw, 1, M.PCM, featout))
        assert base["row_crc"] == got["scoring"][model + "/identity"]["row_crc"], model
        assert got["scoring"][model + "/two_class"]["row_crc"] \
            == got["scoring"][model + "/mild"]["row_crc"], model
    got["scoring"]["en-us_ds2/mild"] = parse_scoring(
        both_ways(exe, "score", S.EN_US, files["mild", "3x13"], "-", 2, M.PCM, featout))
    return got, fr_feat, files


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        scale, out = 1.0, None
        while out is None:
            out = generate(tmp, scale)
            if out is None:
                print("no hypothesis or no alignment at scale %g: halved" % scale)
                scale /= 2
                assert scale > 1e-3
        got, fr_feat, files = out
        texts = {os.path.basename(p): open(p, encoding="ascii").read() for p in files.values()}
    if check:
        bad = []
        have = M.results() if os.path.exists(M.RESULTS_JSON) and os.path.exists(M.ROWS_NPZ) else {}
        got = json.loads(json.dumps(got))
        for sect in sorted(set(got) | set(have)):
            a, b = got.get(sect), have.get(sect)
            if isinstance(a, dict) and isinstance(b, dict):
                bad += [sect + "." + k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            elif a != b:
                bad.append(sect)
        for name, text in texts.items():
            p = os.path.join(M.MLLR_DIR, name)
            if not os.path.exists(p) or open(p, encoding="ascii").read() != text:
                bad.append(name)
        if not os.path.exists(M.FR_FEAT) or not np.array_equal(np.load(M.FR_FEAT), fr_feat):
            bad.append(os.path.basename(M.FR_FEAT))
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    os.makedirs(M.MLLR_DIR, exist_ok=True)
    for name, text in texts.items():
        with open(os.path.join(M.MLLR_DIR, name), "w", encoding="ascii") as fh:
            fh.write(text)
    np.save(M.FR_FEAT, fr_feat)
    got, rows = M.split_rows(got)
    np.savez_compressed(M.ROWS_NPZ, **rows)
    with open(M.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d scoring cases, scale %g, %d + %d bytes" % (len(got["scoring"]), got["scale"],
                                                        os.path.getsize(M.RESULTS_JSON),
                                                        os.path.getsize(M.ROWS_NPZ)))


if __name__ == "__main__":
    main()
