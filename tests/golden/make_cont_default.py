#!/usr/bin/env python3
"""Writes tests/golden/cont_default_results.json: the reference library, in its DEFAULT
configuration (compallsen = no), recognising and aligning goforward.raw with the continuous
models C3 and C1 of tests/cont_common (built afresh from en-us into a temporary directory) --
the truth the *_active entry points are tested against on an enabled continuous model
(tests/test_gpu_cont_default.py).

It compiles the drivers under tests/harness/ against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs them with no setting but loglevel (and "no" where a
driver takes COMPALLSEN, which leaves the key unset).  Per model the file holds:

    rec.<grammar>   goforward, loop, nulls, loop400 (fsg_default_driver.c) and turtle
                    (jsgf_driver.c, the public rule): frames, hyp, score, segments [word, sf, ef,
                    ascr, lscr, prob], json (decoder_result_json(d, 0, 0)), errors (what the
                    library logged at loglevel=ERROR, file and line stripped)
    align           the text "go forward ten meters" (cont_default_driver.c): frames, json0, json1,
                    json2 (null where decoder_result_json gave NULL), errors
    rec_align       goforward recognised, then aligned (fsg_align_driver.c): frames, hyp, score,
                    json0, json1, json2, errors

    python tests/golden/make_cont_default.py           # rewrite the fixture
    python tests/golden/make_cont_default.py --check   # rewrite nothing; exit 1 and name what would change
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

RESULTS_JSON = os.path.join(CC.GOLD, "cont_default_results.json")
PCM = os.path.join(CC.GOLD, "goforward.raw")
MODELS = ("C3", "C1")
FSGS = ("goforward", "loop", "nulls", "loop400")
JSGF = "turtle"
TEXT = "go forward ten meters"
DRIVERS = ("fsg_default_driver", "jsgf_driver", "fsg_align_driver", "cont_default_driver")


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)


def build_drivers(tmp):
    exe = {}
    for name in DRIVERS:
        exe[name] = os.path.join(tmp, name)
        subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                        "-I" + reference.BUILD, os.path.join(ROOT, "tests", "harness", name + ".c"),
                        reference.LIBRARY, "-lm", "-o", exe[name]], check=True)
    return exe


def run(*argv):
    """a driver's lines as {tag: [rest, ...]} and the library's error log"""
    r = subprocess.run([str(a) for a in argv], check=True, capture_output=True, encoding="utf-8")
    out = {}
    for line in r.stdout.splitlines(keepends=True):
        tag, _, rest = line.partition(" ")
        out.setdefault(tag.rstrip("\n"), []).append(rest)
    errors = [re.sub(r'^ERROR: "[^"]*", line \d+: ', "", line) for line in r.stderr.splitlines()]
    return out, errors


def _hyp(out, rec):
    rec["hyp"] = rec["score"] = None
    if "HYP" in out:
        score, _, text = out["HYP"][0].rstrip("\n").partition(" ")
        rec["hyp"], rec["score"] = text, int(score)


def parse_rec(out, errors):
    rec = {"frames": int(out["FRAMES"][0]), "segments": [], "json": out["JSON"][0], "errors": errors}
    _hyp(out, rec)
    for rest in out.get("SEG", []):
        t = rest.rstrip("\n").split(" ", 5)
        rec["segments"].append([t[5]] + [int(x) for x in t[:5]])
    return rec


def parse_levels(out, errors):
    rec = {"frames": int(out["FRAMES"][0]), "errors": errors}
    for level in "012":
        line = out["JSON" + level][0]
        rec["json" + level] = None if line.strip() == "NOALIGN" else line
    return rec


def generate(tmp):
    exe = build_drivers(tmp)
    got = {}
    for model in MODELS:
        d = CC.BUILDERS[model](os.path.join(tmp, model))
        rec = {}
        for g in FSGS:
            rec[g] = parse_rec(*run(exe["fsg_default_driver"], d, os.path.join(CC.GOLD, "fsg", g + ".fsg"),
                                    PCM, 0))
        rec[JSGF] = parse_rec(*run(exe["jsgf_driver"], d, os.path.join(CC.GOLD, "jsgf", JSGF + ".gram"),
                                   PCM, 0, "no", "-"))
        out, errors = run(exe["fsg_align_driver"], d, os.path.join(CC.GOLD, "fsg", "goforward.fsg"),
                          PCM, 0, "no")
        ra = parse_levels(out, errors)
        _hyp(out, ra)
        got[model] = {"rec": rec, "align": parse_levels(*run(exe["cont_default_driver"], "align", d,
                                                             PCM, TEXT)),
                      "rec_align": ra}
    return got


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        got = generate(tmp)
    if check:
        have = results() if os.path.exists(RESULTS_JSON) else {}
        bad = []
        for m in sorted(set(got) | set(have)):
            a, b = got.get(m, {}), have.get(m, {})
            for sect in sorted(set(a) | set(b)):
                if a.get(sect) != b.get(sect):
                    bad.append(m + "." + sect)
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(got)} models, {os.path.getsize(RESULTS_JSON)} bytes")


if __name__ == "__main__":
    main()
