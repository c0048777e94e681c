#!/usr/bin/env python3
"""Writes tests/golden/jsgf/loop200.gram, tests/golden/jsgf_results.json and
tests/golden/jsgf_fsg_texts.json.gz: the reference library
parsing the JSGF grammars under tests/golden/jsgf/, building the FSG of a rule and recognising the
committed recordings against it -- the truth that ssw_jsgf_* and the grammar search over
JSGF-born grammars are tested against.

It compiles tests/harness/jsgf_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it twice per case of tests/jsgf_common.CASES: with
compallsen=yes, and with no setting but loglevel.  Per case the files hold (fsg, fsg_second and
fsg_search, lists of lines, in the .json.gz; everything else in the .json):

    group, grammar, model, recording, samples, toprule   the case as jsgf_common lists it
    name       jsgf_grammar_name
    rules      [name, public] in jsgf_rule_iter order, internal rules included
    chosen     the rule built: -toprule through jsgf_get_rule, else jsgf_get_public_rule
    refused    the step that failed ("Start rule halt not found", "decoder_set_fsg"), or null
    fsg        fsg_model_write after jsgf_build_fsg
    fsg_second the same of a second jsgf_build_fsg of the rule from the same parsed grammar (the
               weights are normalised in place, again)
    fsg_search fsg_model_write after decoder_set_fsg: silences, fillers and alternates added
    yes, default   per configuration: frames, hyp, score, segments ([word, sf, ef, ascr, lscr,
               prob]), json (decoder_result_json(d, 0, 0), the line with its newline), errors
               (what the library logged at loglevel=ERROR, file and line stripped)

    python tests/golden/make_jsgf.py           # rewrite loop200.gram and the fixture
    python tests/golden/make_jsgf.py --check   # rewrite nothing; exit 1 and name what would change
"""
import gzip
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import jsgf_common as C  # noqa: E402

MODELS = os.path.join(ROOT, "soundswallower_amd", "model")


def build_driver(tmp):
    exe = os.path.join(tmp, "jsgf_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "jsgf_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def run_config(exe, case, config):
    name, group, grammar, model, recording, samples, toprule = case
    r = subprocess.run([exe, os.path.join(MODELS, model), C.gram_path(grammar),
                        os.path.join(C.GOLD, recording), str(samples), config, toprule or "-"],
                       check=True, capture_output=True, encoding="utf-8")
    top = {"name": None, "rules": [], "chosen": None, "refused": None, "fsg": [], "fsg_second": [],
           "fsg_search": []}
    rec = {"frames": None, "hyp": None, "score": None, "segments": [], "json": None, "errors": []}
    for line in r.stdout.splitlines(keepends=True):
        tag, _, rest = line.partition(" ")
        text = rest.rstrip("\n")
        if tag == "GRAMMAR":
            top["name"] = text
        elif tag == "RULE":
            top["rules"].append([text[2:], text[0] == "1"])
        elif tag == "CHOSEN":
            top["chosen"] = text
        elif tag == "REFUSED":
            top["refused"] = text
        elif tag == "FSG":
            top["fsg"].append(text)
        elif tag == "FSG2":
            top["fsg_second"].append(text)
        elif tag == "FSGX":
            top["fsg_search"].append(text)
        elif tag == "FRAMES":
            rec["frames"] = int(rest)
        elif tag == "HYP":
            score, _, hyp = text.partition(" ")
            rec["hyp"], rec["score"] = hyp, int(score)
        elif tag == "SEG":
            t = text.split(" ", 5)
            rec["segments"].append([t[5]] + [int(x) for x in t[:5]])
        elif tag == "JSON":
            rec["json"] = rest
    for line in r.stderr.splitlines():
        rec["errors"].append(re.sub(r'^ERROR: "[^"]*", line \d+: ', "", line))
    return top, rec


def run_case(exe, case):
    name, group, grammar, model, recording, samples, toprule = case
    out = {"group": group, "grammar": grammar, "model": model, "recording": recording,
           "samples": samples, "toprule": toprule}
    tops = []
    for config in C.CONFIGS:
        top, rec = run_config(exe, case, config)
        tops.append(top)
        out[config] = rec
    if tops[0] != tops[1]:
        sys.exit("%s: the grammar differs between the configurations" % name)
    out.update(tops[0])
    return out


def dumps(o, depth=0):
    """JSON with a line per key of an object and per row of a list of lists (rules, segments)"""
    pad = "\n" + " " * (depth + 1)
    if isinstance(o, dict) and o:
        return ("{" + ",".join(pad + json.dumps(k) + ": " + dumps(o[k], depth + 1) for k in sorted(o))
                + "\n" + " " * depth + "}")
    if isinstance(o, list) and o and isinstance(o[0], list):
        return "[" + ",".join(pad + dumps(x, depth + 1) for x in o) + "\n" + " " * depth + "]"
    return json.dumps(o, ensure_ascii=False)


def generate(tmp):
    exe = build_driver(tmp)
    return {case[0]: run_case(exe, case) for case in C.CASES}


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    loop = C.gram_path("loop200")
    have_loop = open(loop, encoding="utf-8").read() if os.path.exists(loop) else None
    bad = []
    if have_loop != C.loop200_text():
        if check:
            bad.append("loop200.gram")
        else:
            with open(loop, "w", encoding="utf-8") as f:
                f.write(C.loop200_text())
    if check and bad:
        print("differs: loop200.gram")
        sys.exit(1)
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = C.results() if os.path.exists(C.RESULTS_JSON) and os.path.exists(C.TEXTS_GZ) else {}
        bad = [k for k in sorted(set(got) | set(have)) if have.get(k) != got.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    texts = {k: {t: v.pop(t) for t in C.TEXT_KEYS} for k, v in got.items()}
    with open(C.RESULTS_JSON, "w", encoding="utf-8") as f:
        f.write(dumps(got) + "\n")
    # mtime=0, no file name: the same texts give the same bytes
    with open(C.TEXTS_GZ, "wb") as raw, gzip.GzipFile("", "wb", 9, raw, mtime=0) as f:
        f.write(json.dumps(texts, indent=0, sort_keys=True, ensure_ascii=False).encode("utf-8"))
    print(f"{len(got)} cases, {os.path.getsize(C.RESULTS_JSON)} + {os.path.getsize(C.TEXTS_GZ)} bytes")


if __name__ == "__main__":
    main()
