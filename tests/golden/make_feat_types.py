#!/usr/bin/env python3
"""Writes the fixtures of the dynamic-feature tests:

    tests/golden/feat_types/cases.json, types.npz, cmn.npz, lda.npz, chain.npz
        the reference library, built by build() into oracle/_ref/, computing the features of
        every case of tests/feat_types_common.CASES through tests/harness/feat_types_driver.c
        (feat_init from the settings, feat_s2mfc2feat_live with beginutt = endutt = 1 per
        utterance): per case the rows and, with a CMN, the state after every utterance.
          cases.<name>   file, settings (the LDA file by its name), lens, mode, input,
                         dims {width, raw, window, streams, ceplen, has_cmn}
          e2e            model C1-lda (feat_types_common.model_c1_lda_dir, built afresh into a
                         temporary directory) through tests/harness/cont_driver.c:
                         rec {scorer, frames, hyp, score, segments, json} for goforward.fsg and
                         align {scorer, json} (align_level 1) of "go forward ten meters"
    tests/golden/feat_types/feature_transform is the reference's tests/data/feature_transform
    (data: one 36 x 39 matrix), copied once by hand; --check compares it when the tree is there.

    python tests/golden/make_feat_types.py           # rewrite the fixtures
    python tests/golden/make_feat_types.py --check   # rewrite nothing; exit 1 and name what would change
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
from tests import feat_types_common as FT  # noqa: E402
from tests.golden.make_cont import build_driver as build_cont_driver  # noqa: E402
from tests.golden.make_sc import parse_rec, run  # noqa: E402

PCM = os.path.join(CC.GOLD, "goforward.raw")
FSG = os.path.join(CC.GOLD, "fsg", "goforward.fsg")
LIMIT = os.path.getsize(CC.ROWS_NPZ)    # the largest fixture of this kind


def build_driver(tmp):
    exe = os.path.join(tmp, "feat_types_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-ffp-contract=off",
                    "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "feat_types_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def record(exe, tmp, name, case):
    cep = FT.case_input(case)
    fin, fout = os.path.join(tmp, name + ".cep"), os.path.join(tmp, name + ".out")
    cep.astype("<f4").tofile(fin)
    args = [exe, case["mode"], fin, fout] + ["%s=%s" % kv for kv in sorted(case["settings"].items())] \
        + ["--"] + [str(n) for n in case["lens"]]
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit("%s: %s\n%s" % (name, " ".join(args), r.stderr[-2000:]))
    width, raw, window, streams, ceplen, has_cmn = (int(x) for x in r.stdout.split()[1:7])
    blob = np.fromfile(fout, "<f4")
    rows, state, nframe, at = [], [], [], 0
    for n in case["lens"]:
        rows.append(blob[at:at + n * width])
        at += n * width
        if has_cmn:
            state.append(blob[at:at + 2 * ceplen])
            nframe.append(blob[at + 2 * ceplen:at + 2 * ceplen + 1].view("<i4")[0])
            at += 2 * ceplen + 1
    assert at == len(blob), name
    meta = {"file": case["file"], "settings": FT.portable(case["settings"]), "lens": case["lens"],
            "mode": case["mode"], "input": case["input"],
            "dims": {"width": width, "raw": raw, "window": window, "streams": streams,
                     "ceplen": ceplen, "has_cmn": has_cmn}}
    arrays = {name: np.concatenate(rows).astype("<f4")}
    if has_cmn:
        arrays[name + ".state"] = np.stack(state).astype("<f4")
        arrays[name + ".nframe"] = np.array(nframe, "<i4")
    return meta, arrays


def generate(tmp):
    exe = build_driver(tmp)
    meta, files = {}, {}
    for name, case in FT.CASES.items():
        meta[name], arrays = record(exe, tmp, name, case)
        files.setdefault(case["file"], {}).update(arrays)
    cont = build_cont_driver(tmp)
    d = FT.model_c1_lda_dir(os.path.join(tmp, "C1-lda"))
    rec = parse_rec(run(cont, "rec", d, FSG, PCM))
    assert rec["hyp"], "the reference finds no hypothesis under C1-lda: drop other columns"
    a = parse_rec(run(cont, "align", d, PCM))
    return {"cases": meta, "e2e": {"rec": rec, "align": {"scorer": a["scorer"], "json": a["json"]}}}, files


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got, files = generate(tmp)
    got = json.loads(json.dumps(got))
    if check:
        bad = []
        have = {}
        if os.path.exists(FT.CASES_JSON):
            with open(FT.CASES_JSON, encoding="utf-8") as fh:
                have = json.load(fh)
        for sect in ("cases", "e2e"):
            a, b = got.get(sect, {}), have.get(sect, {})
            bad += [sect + "." + k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        for f, arrays in files.items():
            path = os.path.join(FT.DIR, f + ".npz")
            z = np.load(path) if os.path.exists(path) else None
            for k, v in arrays.items():
                if z is None or k not in z.files or z[k].tobytes() != v.tobytes():
                    bad.append(f + ".npz:" + k)
        src = reference.source_tree()
        ours = os.path.join(FT.DIR, "feature_transform")
        theirs = os.path.join(src, "tests", "data", "feature_transform") if src else None
        if theirs and os.path.exists(theirs) and open(theirs, "rb").read() != open(ours, "rb").read():
            bad.append("feature_transform")
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    os.makedirs(FT.DIR, exist_ok=True)
    for f, arrays in files.items():
        path = os.path.join(FT.DIR, f + ".npz")
        np.savez_compressed(path, **arrays)
        assert os.path.getsize(path) < LIMIT, "%s: %d bytes" % (path, os.path.getsize(path))
        print("%s: %d arrays, %d bytes" % (path, len(arrays), os.path.getsize(path)))
    with open(FT.CASES_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, separators=(",", ":"), sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print("%d cases; hyp %r" % (len(got["cases"]), got["e2e"]["rec"]["hyp"]))


if __name__ == "__main__":
    main()
