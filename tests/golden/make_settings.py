#!/usr/bin/env python3
"""Writes the fixtures of the non-default logbase / varfloor / mixwfloor / tmatfloor tests:

    tests/golden/settings_results.json, tests/golden/settings/rows.npz (the whole rows, int16)
        the reference library, built by build() into oracle/_ref/, scoring, aligning and
        recognising tests/golden/goforward.raw through tests/harness/settings_driver.c with
        compallsen = yes and the settings of tests/settings_common:
          scoring.<case>  scorer, det_crc, var_crc, frames, row_crc [frames], n_floored (the
                          count the reference's loader logs), settings, model, and
                          rows {frame: [n_sen]} for frames 0, 1, 2 and the last
          flows.<case>    align: scorer, json (align_level 1)
                          rec:   scorer, frames, hyp, score, segments, json, of
                                 tests/golden/fsg/goforward.fsg
                          rec_chain: the same of the text's chain grammar (settings_common.chain_fsg)
    fr-mixw (fr-fr with synthesised mixture weights and no sendump) is made afresh in a temporary
    directory.  The features the reference scored are the committed ones (en-us's:
    tests/golden/sc/goforward_feat.npy, fr-fr's: tests/golden/mllr/goforward_fr_feat.npy):
    checked here, so no features are committed twice.

    python tests/golden/make_settings.py           # rewrite the fixtures
    python tests/golden/make_settings.py --check   # rewrite nothing; exit 1 and name what would change
"""
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import settings_common as SC  # noqa: E402
from tests.golden.make_sc import parse_rec, parse_scoring  # noqa: E402


def build_driver(tmp):
    exe = os.path.join(tmp, "settings_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "settings_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def run(exe, mode, hmm, over, *args):
    s = SC.settings(over)
    r = subprocess.run([exe, mode, hmm] + [repr(float(s[k])) for k in SC.KEYS] + [str(a) for a in args],
                       check=True, capture_output=True, encoding="utf-8")
    return r.stdout.splitlines(keepends=True), r.stderr


def generate(tmp):
    exe = build_driver(tmp)
    dirs = {"en-us": SC.EN_US, "fr-mixw": SC.fr_mixw_dir(os.path.join(tmp, "fr-mixw"))}
    featout = os.path.join(tmp, "feat.f32")
    got = {"scoring": {}, "flows": {}}
    for case, (model, over) in SC.SCORING.items():
        lines, log = run(exe, "score", dirs[model], over, SC.PCM, featout)
        rec = parse_scoring(lines)
        assert np.array_equal(SC.features(model), np.fromfile(featout, "<f4").reshape(-1, 39)), \
            "the reference's feature rows are not the committed ones of " + model
        floored = re.findall(r"(\d+) variance values floored", log)
        assert len(floored) == 1, "the reference logged %d counts of floored variances" % len(floored)
        rec["n_floored"] = int(floored[0])
        rec["model"], rec["settings"] = model, SC.settings(over)
        got["scoring"][case] = rec
    for case, (kind, model, over) in SC.FLOWS.items():
        if kind == "align":
            a = parse_rec(run(exe, "align", dirs[model], over, SC.PCM)[0])
            got["flows"][case] = {"scorer": a["scorer"], "json": a["json"]}
        else:
            fsg = SC.FSG if kind == "rec" else SC.chain_fsg(os.path.join(tmp, "chain.fsg"))
            got["flows"][case] = parse_rec(run(exe, "rec", dirs[model], over, fsg, SC.PCM)[0])
            assert got["flows"][case]["hyp"], "no hypothesis for " + case
        got["flows"][case]["model"], got["flows"][case]["settings"] = model, SC.settings(over)
    return got


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = SC.results() if os.path.exists(SC.RESULTS_JSON) and os.path.exists(SC.ROWS_NPZ) else {}
        got = json.loads(json.dumps(got))
        bad = []
        for sect in sorted(set(got) | set(have)):
            a, b = got.get(sect, {}), have.get(sect, {})
            bad += [sect + "." + k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    got, rows = SC.split_rows(got)
    os.makedirs(os.path.dirname(SC.ROWS_NPZ), exist_ok=True)
    np.savez_compressed(SC.ROWS_NPZ, **rows)
    with open(SC.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d scoring cases, %d flows, %d + %d bytes"
          % (len(got["scoring"]), len(got["flows"]), os.path.getsize(SC.RESULTS_JSON),
             os.path.getsize(SC.ROWS_NPZ)))


if __name__ == "__main__":
    main()
