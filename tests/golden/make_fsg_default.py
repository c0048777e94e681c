#!/usr/bin/env python3
"""Writes tests/golden/fsg_default_results.json: the reference library, in its DEFAULT
configuration (compallsen = no), recognising the committed recordings against the word FSGs under
tests/golden/fsg/ -- the truth that ssw_recognize_batch_active is tested against.

It compiles tests/harness/fsg_default_driver.c against the reference library that build() makes
in oracle/_ref/ (oracle/reference.py) and runs it once per case of tests/fsg_common.CASES, with
no setting but loglevel.  The records have the format of make_fsg.py's.  Per case the file holds:

    group, grammar, model, recording, samples   the case as fsg_common lists it
    fsg        fsg_model_write of the grammar as the reference read it: the null transitions
               closed, in the order fsg_model_arcs walks them
    fsg_search the same after decoder_set_fsg: with the silence and filler loops and the alternate
               pronunciations fsg_search_init added
    frames     decoder_n_frames
    hyp        decoder_hyp, or null
    score      its score, or null
    segments   [word, sf, ef, ascr, lscr, prob] of decoder_seg_iter / seg_iter_prob
    json       decoder_result_json(d, 0, 0), the line with its newline
    errors     what the library logged at loglevel=ERROR (file and line stripped)

    python tests/golden/make_fsg_default.py           # rewrite the fixture
    python tests/golden/make_fsg_default.py --check   # rewrite nothing; exit 1 and name every case whose
                                              # record would change
"""
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import fsg_common as C  # noqa: E402

RESULTS_JSON = os.path.join(C.GOLD, "fsg_default_results.json")
MODELS = os.path.join(ROOT, "soundswallower_amd", "model")


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)


def build_driver(tmp):
    exe = os.path.join(tmp, "fsg_default_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "fsg_default_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def run_case(exe, case):
    name, group, grammar, model, recording, samples = case
    r = subprocess.run([exe, os.path.join(MODELS, model), C.fsg_path(grammar),
                        os.path.join(C.GOLD, recording), str(samples)], check=True,
                       capture_output=True, encoding="utf-8")
    rec = {"group": group, "grammar": grammar, "model": model, "recording": recording,
           "samples": samples, "fsg": [], "fsg_search": [], "frames": None, "hyp": None, "score": None,
           "segments": [], "json": None, "errors": []}
    for line in r.stdout.splitlines(keepends=True):
        tag, _, rest = line.partition(" ")
        if tag == "FSG":
            rec["fsg"].append(rest.rstrip("\n"))
        elif tag == "FSGX":
            rec["fsg_search"].append(rest.rstrip("\n"))
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
    for line in r.stderr.splitlines():
        # ERROR: "fsg_search.c", line 915: Final result does not match ...
        rec["errors"].append(re.sub(r'^ERROR: "[^"]*", line \d+: ', "", line))
    return rec


def generate(tmp):
    exe = build_driver(tmp)
    return {case[0]: run_case(exe, case) for case in C.CASES}


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = results() if os.path.exists(RESULTS_JSON) else {}
        bad = [k for k in sorted(set(got) | set(have)) if have.get(k) != got.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(got)} cases, {os.path.getsize(RESULTS_JSON)} bytes")


if __name__ == "__main__":
    main()
