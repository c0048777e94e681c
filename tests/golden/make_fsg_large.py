#!/usr/bin/env python3
"""Writes the large grammars under tests/golden/fsg/ (loop200, loop400, nulls200: more than 4096
phone-tree HMMs each) and tests/golden/fsg_large_results.json: the reference library recognising
goforward.raw against them, whole and cut to 19200 samples -- the truth that the large path of
the grammar search (ssw_grammar_prepare_large) is tested against.

The word lists: `go forward ten meters backward nine`, then the entries of the en-us dict.txt in
file order whose head word is ASCII letters only (str.isalpha()) and has three phones or more --
every 600th of them for the 200-word lists, every 300th for loop400 (the dictionary runs out at
395 words) -- duplicates skipped, cut at the target count.  Every word has probability 1 / n,
printed with %.6f.  nulls200 has the 200 words as 0 -> 1 and the null transitions 1 -> 0 (0.5) and
1 -> 2 (0.5); start 0, final 2.

The records come from tests/harness/fsg_driver.c (compallsen=yes, default beams) against the
reference library in oracle/_ref/, in the format of make_fsg.py's.

    python tests/golden/make_fsg_large.py           # rewrite the grammars and the fixture
    python tests/golden/make_fsg_large.py --check   # rewrite nothing; exit 1 and name every
                                                    # grammar and case that would change
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import reference  # noqa: E402
from tests import fsg_common as C  # noqa: E402
from tests import fsg_large_common as CL  # noqa: E402
import make_fsg  # noqa: E402

DICT = os.path.join(make_fsg.MODELS, "en-us", "dict.txt")
FIRST = "go forward ten meters backward nine".split()


def candidates():
    out = []
    with open(DICT, encoding="utf-8") as f:
        for line in f:
            t = line.split()
            if len(t) >= 4 and t[0].isascii() and t[0].isalpha():
                out.append(t[0])
    return out


def word_list(cand, n, step):
    words = []
    for w in FIRST + cand[::step]:
        if w not in words:
            words.append(w)
        if len(words) == n:
            break
    return words


def grammar_text(name, cand):
    n, step, states = CL.GRAMMARS[name]
    words = word_list(cand, n, step)
    every = "every %dth entry of the en-us dictionary" % step
    if states == 1:
        head = ["# a free loop over %d words: six of the recording's, then %s" % (len(words), every),
                "# whose head word is ASCII letters only and has three phones or more, duplicates",
                "# skipped; every word with probability 1 / n (make_fsg_large.py)"]
    else:
        head = ["# %d words from state 0 to state 1 -- six of the recording's, then %s"
                % (len(words), every),
                "# whose head word is ASCII letters only and has three phones or more, duplicates",
                "# skipped, every word with probability 1 / n -- and the null transitions 1 -> 0 and",
                "# 1 -> 2: a (NULL) entry after every word (make_fsg_large.py)"]
    to = 0 if states == 1 else 1
    lines = head + ["FSG_BEGIN " + name, "NUM_STATES %d" % states, "START_STATE 0",
                    "FINAL_STATE %d" % (states - 1)]
    lines += ["TRANSITION 0 %d %.6f %s" % (to, 1.0 / len(words), w) for w in words]
    if states == 3:
        lines += ["TRANSITION 1 0 0.5", "TRANSITION 1 2 0.5"]
    return "\n".join(lines + ["FSG_END"]) + "\n"


def read(path):
    if not os.path.exists(path):
        return None
    with open(path, encoding="utf-8") as f:
        return f.read()


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    cand = candidates()
    texts = {g: grammar_text(g, cand) for g in CL.GRAMMARS}
    bad = ["grammar " + g for g in sorted(texts) if read(C.fsg_path(g)) != texts[g]]
    if not check:
        for g, text in texts.items():
            with open(C.fsg_path(g), "w", encoding="utf-8") as f:
                f.write(text)
    elif bad:  # (the driver would read other grammars than the rule's)
        for k in bad:
            print("differs:", k)
        sys.exit(1)
    with tempfile.TemporaryDirectory() as tmp:
        exe = make_fsg.build_driver(tmp)
        got = {case[0]: make_fsg.run_case(exe, case) for case in CL.CASES}
    if check:
        have = CL.results() if os.path.exists(CL.RESULTS_JSON) else {}
        bad = [k for k in sorted(set(got) | set(have)) if have.get(k) != got.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(CL.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(got)} cases, {os.path.getsize(CL.RESULTS_JSON)} bytes")


if __name__ == "__main__":
    main()
