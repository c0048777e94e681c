#!/usr/bin/env python3
"""Writes the fixtures of the continuous-density (one codebook per senone) tests:

    tests/golden/cont_results.json, tests/golden/cont/rows.npz (the whole rows, int16)
        the reference library, built by build() into oracle/_ref/, scoring with the models C3,
        C3-ties and C1 of tests/cont_common (built afresh from en-us into a temporary directory)
        through tests/harness/cont_driver.c, and recognising and aligning with C3:
          scoring.<case>  scorer, det_crc, var_crc, frames, row_crc [frames],
                          rows {frame: [n_sen]} for frames 0, 1, 2 and the last, and the case's
                          settings; cases: cont_common.CASES
          rec.<grammar>   scorer, frames, hyp, score, segments, json   (compallsen = yes)
          align           scorer, json (align_level 1)
          scale           the factor the features of C3_scaled are multiplied by
    K = 8 densities: the reference finds a hypothesis under C3 for all three grammars.
    The features are those of tests/golden/sc/goforward_feat.npy (en-us's front end): checked here.
    C3_scaled goes through the driver's inject mode; at least one raw score of frames 0, 1, 2 and
    the last has to leave int16 before the clamp (the restatement says), else the factor is doubled.
    At 40 every one of them does: the frame's best clamps too and the recorded rows are all 0.

    python tests/golden/make_cont.py           # rewrite the fixtures
    python tests/golden/make_cont.py --check   # rewrite nothing; exit 1 and name what would change
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
from tests import cont_common as CC  # noqa: E402
from tests.golden.make_sc import parse_rec, parse_scoring, run  # noqa: E402

PCM = os.path.join(CC.GOLD, "goforward.raw")
GRAMMARS = ("goforward", "loop", "nulls")
SCALE = 40


def build_driver(tmp):
    exe = os.path.join(tmp, "cont_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "cont_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def clamps(d, topn, aw, mixwfloor, feats):
    """does a raw score of the first three frames or the last leave int16 (the restatement says)"""
    import soundswallower_amd as ssw
    m = ssw.Model(**CC.model_paths(d), config={"device": ssw.SSW_DEVICE_NONE, "topn": topn, "aw": aw,
                                               "mixwfloor": mixwfloor})
    raw = CC.restated_from_model(m, aw=aw).score(feats[[0, 1, 2, -1]], unclamped=True)
    m.close()
    n = int(np.count_nonzero((raw // aw > 32767) | (raw // aw < -32768)))
    print("scaled features: %d of %d raw scores clamp" % (n, raw.size))
    return n > 0


def generate(tmp):
    exe = build_driver(tmp)
    dirs = {n: b(os.path.join(tmp, n)) for n, b in CC.BUILDERS.items()}
    feats = CC.features()
    featout = os.path.join(tmp, "feat.f32")
    got = {"scoring": {}, "rec": {}, "align": None, "scale": None}
    for case, (model, topn, aw, mixwfloor, scale) in CC.CASES.items():
        if scale == 1:
            rec = parse_scoring(run(exe, "score", dirs[model], topn, aw, repr(mixwfloor), PCM, featout))
            assert np.array_equal(feats, np.fromfile(featout, "<f4").reshape(-1, 39)), \
                "the reference's feature rows are not tests/golden/sc/goforward_feat.npy"
        else:
            factor = SCALE
            while True:
                fin = os.path.join(tmp, "scaled.f32")
                (feats * np.float32(factor)).astype("<f4").tofile(fin)
                rec = parse_scoring(run(exe, "inject", dirs[model], topn, aw, repr(mixwfloor), fin,
                                        len(feats)))
                if clamps(dirs[model], topn, aw, mixwfloor, feats * np.float32(factor)):
                    break
                factor *= 2
                assert factor < 1 << 20
            got["scale"] = factor
        rec["settings"] = {"model": model, "topn": topn, "aw": aw, "mixwfloor": mixwfloor}
        got["scoring"][case] = rec
    for g in GRAMMARS:
        got["rec"][g] = parse_rec(run(exe, "rec", dirs["C3"], os.path.join(CC.GOLD, "fsg", g + ".fsg"),
                                      PCM))
        assert got["rec"][g]["hyp"], "no hypothesis for %s under C3: raise K" % g
    a = parse_rec(run(exe, "align", dirs["C3"], PCM))
    got["align"] = {"scorer": a["scorer"], "json": a["json"]}
    return got


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = CC.results() if os.path.exists(CC.RESULTS_JSON) and os.path.exists(CC.ROWS_NPZ) else {}
        bad = []
        got = json.loads(json.dumps(got))
        for sect in sorted(set(got) | set(have)):
            a, b = got.get(sect), have.get(sect)
            if isinstance(a, dict) and isinstance(b, dict) and sect != "align":
                bad += [sect + "." + k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
            elif a != b:
                bad.append(sect)
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    got, rows = CC.split_rows(got)
    os.makedirs(os.path.dirname(CC.ROWS_NPZ), exist_ok=True)
    np.savez_compressed(CC.ROWS_NPZ, **rows)
    with open(CC.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d scoring cases, %d + %d bytes" % (len(got["scoring"]), os.path.getsize(CC.RESULTS_JSON),
                                             os.path.getsize(CC.ROWS_NPZ)))


if __name__ == "__main__":
    main()
