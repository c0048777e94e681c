#!/usr/bin/env python3
"""Writes tests/golden/fsg_align_results.json: the reference library recognising the committed
recordings against grammars and then aligning what it recognised -- decoder_result_json at
align_level 1 and 2 and the entries of decoder_alignment (src/decoder.c:737-798) -- in both of its
configurations: the truth that ssw_recognition_set_align, ssw_recognize_align_batch (compallsen =
yes) and ssw_recognize_align_batch_active (compallsen = no, the library's default) are tested
against.

It compiles tests/harness/fsg_align_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it once per case and configuration of
tests/fsg_align_common.py.  The semi-continuous and the continuous model are laid out afresh in a
temporary directory (tests/sc_common.model_a_dir, tests/cont_common.BUILDERS).  Per record
(key: case "/" configuration):

    kind, grammar, model, recording, samples, config   the case as fsg_align_common lists it
    frames     decoder_n_frames
    hyp        decoder_hyp, or null
    score      its score, or null
    json0      decoder_result_json(d, 0, 0), the line with its newline
    json1      decoder_result_json(d, 0, 1), or null where it returned NULL (no alignment)
    json2      decoder_result_json(d, 0, 2), or null
    words, phones, states
               [name, start, duration, score] of every entry of decoder_alignment, through
               alignment_words / _phones / _states; null without an alignment
    errors     what the library logged at loglevel=ERROR (file and line stripped)

    python tests/golden/make_fsg_align.py           # rewrite the fixture
    python tests/golden/make_fsg_align.py --check   # rewrite nothing; exit 1 and name every record
                                                    # that would change
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
from tests import cont_common as CC  # noqa: E402
from tests import fsg_align_common as A  # noqa: E402
from tests import fsg_common as C  # noqa: E402
from tests import sc_common as S  # noqa: E402

MODELS = os.path.join(ROOT, "soundswallower_amd", "model")


def build_driver(tmp):
    exe = os.path.join(tmp, "fsg_align_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "fsg_align_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def model_dirs(tmp):
    dirs = {"cb41": S.model_a_dir(os.path.join(tmp, "cb41")),
            "C3": CC.BUILDERS["C3"](os.path.join(tmp, "C3"))}
    return lambda model: dirs.get(model) or os.path.join(MODELS, model)


def run_case(exe, case, config, model_dir):
    name, kind, grammar, model, recording, samples = case
    r = subprocess.run([exe, model_dir(model), A.grammar_path(case), os.path.join(C.GOLD, recording),
                        str(samples), config], check=True, capture_output=True, encoding="utf-8")
    rec = {"kind": kind, "grammar": grammar, "model": model, "recording": recording,
           "samples": samples, "config": config, "frames": None, "hyp": None, "score": None,
           "json0": None, "json1": None, "json2": None, "words": None, "phones": None,
           "states": None, "errors": []}
    levels = {"WORD": "words", "PHONE": "phones", "STATE": "states"}
    for line in r.stdout.splitlines(keepends=True):
        tag, _, rest = line.partition(" ")
        if tag == "FRAMES":
            rec["frames"] = int(rest)
        elif tag == "HYP":
            score, _, text = rest.rstrip("\n").partition(" ")
            rec["hyp"], rec["score"] = text, int(score)
        elif tag in ("JSON0", "JSON1", "JSON2"):
            rec[tag.lower()] = None if rest == "NOALIGN\n" else rest
        elif tag in levels:
            t = rest.rstrip("\n").split(" ", 3)
            if rec[levels[tag]] is None:
                rec["words"], rec["phones"], rec["states"] = (rec[k] or [] for k in
                                                              ("words", "phones", "states"))
            rec[levels[tag]].append([t[3]] + [int(x) for x in t[:3]])
    for line in r.stderr.splitlines():
        rec["errors"].append(re.sub(r'^ERROR: "[^"]*", line \d+: ', "", line))
    return rec


def generate(tmp):
    exe = build_driver(tmp)
    model_dir = model_dirs(tmp)
    got = {}
    for case in A.CASES:
        for config in A.configs(case):
            got[case[0] + "/" + config] = run_case(exe, case, config, model_dir)
    # what was seen of the reference before this fixture existed: without it nothing is pinned
    for config in A.CONFIGS:
        for name in A.ALIGNED:
            rec = got[name + "/" + config]
            assert rec["hyp"] and rec["json1"] and rec["json2"] and rec["states"], (name, config)
        for name in A.NO_HYP:
            rec = got[name + "/" + config]
            assert rec["hyp"] is None and rec["json1"] is None and rec["json2"] is None \
                and rec["words"] is None, (name, config)
        assert len(got["goforward/" + config]["json2"].encode()) == 3509
    assert got["fr/no"]["hyp"] and got["fr/no"]["json1"]
    return got


def dump(got, f):
    """one record per line: the lines of a record are long lists of numbers nobody reads"""
    f.write("{\n")
    f.write(",\n".join(json.dumps(k) + ": " + json.dumps(got[k], sort_keys=True, ensure_ascii=False)
                       for k in sorted(got)))
    f.write("\n}\n")


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = A.results() if os.path.exists(A.RESULTS_JSON) else {}
        bad = [k for k in sorted(set(got) | set(have)) if have.get(k) != got.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(A.RESULTS_JSON, "w", encoding="utf-8") as f:
        dump(got, f)
    print(f"{len(got)} records, {os.path.getsize(A.RESULTS_JSON)} bytes")
    for k in sorted(got):
        print(k, got[k]["frames"], got[k]["hyp"], got[k]["score"],
              "aligned" if got[k]["json1"] else "NOALIGN")


if __name__ == "__main__":
    main()
