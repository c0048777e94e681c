#!/usr/bin/env python3
"""Writes the fixtures of the s2_semi (single-codebook) tests:

    tests/golden/sc/en-us-cb41/{means,variances,feat_params.json}
        model A: our own en-us files with means and variances cut down to codebook 41
        (tests/sc_common.cut_codebook); every other file of the model is en-us's, used by path
    tests/golden/sc/goforward_feat.npy
        the 278 feature rows the reference's acmod scored for tests/golden/goforward.raw with
        model A's front end settings (float32 [278][39])
    tests/golden/sc_results.json, tests/golden/sc/rows.npz (the whole rows, int16)
        the reference library, built by build() into oracle/_ref/, scoring with models A, A-ties
        and B (tests/sc_common) through tests/harness/sc_driver.c, and recognising and aligning
        with model A:
          scoring.<case>  scorer, det_crc, var_crc, frames, row_crc [frames],
                          rows {frame: [n_sen]} for frames 0, 1, 2 and the last
                          cases: A, A-ties, B, and A_topn<N>_ds<D> for the settings of
                          sc_common.SETTINGS
          rec.<grammar>.<yes|no>   scorer, frames, hyp, score, segments, json
          align.<yes|no>           scorer, json (align_level 1)

    python tests/golden/make_sc.py           # rewrite the fixtures
    python tests/golden/make_sc.py --check   # rewrite nothing; exit 1 and name what would change
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
from tests import sc_common as S  # noqa: E402

PCM = os.path.join(S.GOLD, "goforward.raw")
GRAMMARS = ("goforward", "loop", "nulls")


def build_driver(tmp):
    exe = os.path.join(tmp, "sc_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "sc_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def run(exe, *args):
    r = subprocess.run([exe] + [str(a) for a in args], check=True, capture_output=True,
                       encoding="utf-8")
    return r.stdout.splitlines(keepends=True)


def parse_scoring(lines):
    rec = {"scorer": None, "det_crc": None, "var_crc": None, "row_crc": [], "rows": {}}
    for line in lines:
        t = line.split()
        if t[0] == "SCORER":
            rec["scorer"] = t[1]
        elif t[0] == "TABLE":
            rec["det_crc"], rec["var_crc"] = int(t[2]), int(t[4])
        elif t[0] == "ROW":
            assert int(t[1]) == len(rec["row_crc"])
            rec["row_crc"].append(int(t[2]))
        elif t[0] == "FULL":
            rec["rows"][t[1]] = [int(x) for x in t[2:]]
    rec["frames"] = len(rec["row_crc"])
    return rec


def parse_rec(lines):
    rec = {"scorer": None, "frames": None, "hyp": None, "score": None, "segments": [], "json": None}
    for line in lines:
        tag, _, rest = line.partition(" ")
        if tag == "SCORER":
            rec["scorer"] = rest.strip()
        elif tag == "FRAMES":
            rec["frames"] = int(rest)
        elif tag == "HYP":
            score, _, text = rest.rstrip("\n").partition(" ")
            rec["hyp"], rec["score"] = text, int(score)
        elif tag == "SEG":
            t = rest.rstrip("\n").split(" ", 5)
            rec["segments"].append([t[5]] + [int(x) for x in t[:5]])
        elif tag == "JSON":
            rec["json"] = rest
    return rec


def model_a_files(tmp):
    """{name: bytes} of the committed cut, made afresh from en-us"""
    out = {}
    for n in ("means", "variances"):
        p = os.path.join(tmp, "cut_" + n)
        S.cut_codebook(os.path.join(S.EN_US, n), p)
        with open(p, "rb") as fh:
            out[n] = fh.read()
    with open(os.path.join(S.EN_US, "feat_params.json"), "rb") as fh:
        out["feat_params.json"] = fh.read()
    return out


def generate(tmp, cut):
    """(results, feature rows) from the reference; `cut`: model A's files as model_a_files gives
    them (the committed ones need not exist yet)"""
    exe = build_driver(tmp)
    a = os.path.join(tmp, "A")
    os.makedirs(a)
    S._link_shared(a, S.SHARED + ("sendump",))
    for n, blob in cut.items():
        with open(os.path.join(a, n), "wb") as fh:
            fh.write(blob)
    # (model_a_ties_dir and model_b_dir read the committed cut: point them at this one)
    committed = S.MODEL_A
    S.MODEL_A = a
    try:
        ties = S.model_a_ties_dir(os.path.join(tmp, "A-ties"))
        b = S.model_b_dir(os.path.join(tmp, "B"))
    finally:
        S.MODEL_A = committed
    featout = os.path.join(tmp, "feat.f32")
    got = {"scoring": {}, "rec": {}, "align": {}}
    got["scoring"]["A"] = parse_scoring(run(exe, "score", a, 4, 1, PCM, featout))
    feats = np.fromfile(featout, "<f4").reshape(-1, 39)
    got["scoring"]["A-ties"] = parse_scoring(run(exe, "score", ties, 4, 1, PCM, featout))
    assert np.array_equal(feats, np.fromfile(featout, "<f4").reshape(-1, 39))
    for topn, ds in S.SETTINGS:
        got["scoring"]["A_topn%d_ds%d" % (topn, ds)] = parse_scoring(
            run(exe, "score", a, topn, ds, PCM, featout))
    means, _, _ = S.model_b_tables()
    fb = os.path.join(tmp, "featb.f32")
    S.model_b_features(means).astype("<f4").tofile(fb)
    got["scoring"]["B"] = parse_scoring(run(exe, "inject", b, 4, 1, fb, S.B_FRAMES))
    for g in GRAMMARS:
        got["rec"][g] = {c: parse_rec(run(exe, "rec", a, c, os.path.join(S.GOLD, "fsg", g + ".fsg"),
                                          PCM)) for c in ("yes", "no")}
    for c in ("yes", "no"):
        got["align"][c] = parse_rec(run(exe, "align", a, c, PCM))
        got["align"][c] = {"scorer": got["align"][c]["scorer"], "json": got["align"][c]["json"]}
    return got, feats


def main():
    check = "--check" in sys.argv[1:]
    with tempfile.TemporaryDirectory() as tmp:
        cut = model_a_files(tmp)
        bad = []
        for n, blob in cut.items():
            p = os.path.join(S.MODEL_A, n)
            if check:
                if not os.path.exists(p) or open(p, "rb").read() != blob:
                    bad.append("en-us-cb41/" + n)
            else:
                os.makedirs(S.MODEL_A, exist_ok=True)
                with open(p, "wb") as fh:
                    fh.write(blob)
        if not reference.available():
            if check and not bad:
                sys.exit("no reference build in oracle/_ref/ (build() makes it from a "
                         "SoundSwallower tree); the cut of en-us agrees")
            sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower "
                     "tree)")
        got, feats = generate(tmp, cut)
    if check:
        have = S.results() if os.path.exists(S.RESULTS_JSON) and os.path.exists(S.ROWS_NPZ) else {}
        for sect in sorted(set(got) | set(have)):
            for k in sorted(set(got.get(sect, {})) | set(have.get(sect, {}))):
                if have.get(sect, {}).get(k) != json.loads(json.dumps(got.get(sect, {}).get(k))):
                    bad.append(sect + "." + k)
        if not os.path.exists(S.FEAT_A) or not np.array_equal(np.load(S.FEAT_A), feats):
            bad.append("goforward_feat.npy")
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    np.save(S.FEAT_A, feats.astype(np.float32))
    got, rows = S.split_rows(got)
    np.savez_compressed(S.ROWS_NPZ, **rows)
    with open(S.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d scoring cases, %d bytes" % (len(got["scoring"]), os.path.getsize(S.RESULTS_JSON)))


if __name__ == "__main__":
    main()
