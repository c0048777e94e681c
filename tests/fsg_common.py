"""What tests/golden/make_fsg.py records and the grammar tests replay: the recognition cases (a
grammar under tests/golden/fsg/, a model, a recording, a sample count) and the fixture file."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FSG_DIR = os.path.join(GOLD, "fsg")
RESULTS_JSON = os.path.join(GOLD, "fsg_results.json")

# (case, group, grammar, model, recording, samples (0: the whole recording)); the groups are the
# seven rows of mandatory grammars, and one more (see below)
CASES = (
    ("goforward", "goforward", "goforward", "en-us", "goforward.raw", 0),
    ("loop", "loop", "loop", "en-us", "goforward.raw", 0),
    ("nulls", "nulls", "nulls", "en-us", "goforward.raw", 0),
    ("sil", "sil", "sil", "en-us", "goforward.raw", 0),
    ("nomatch", "nomatch", "nomatch", "en-us", "goforward.raw", 0),
    ("fr", "fr", "fr", "fr-fr", "goforward_fr.raw", 0),
    ("goforward_1200ms", "truncations", "goforward", "en-us", "goforward.raw", 19200),
    ("loop_1200ms", "truncations", "loop", "en-us", "goforward.raw", 19200),
    ("goforward_410", "truncations", "goforward", "en-us", "goforward.raw", 410),
    ("loop_410", "truncations", "loop", "en-us", "goforward.raw", 410),
    # beyond the mandatory seven: grammars of more than 1024 and more than 2048 phone-tree HMMs
    # (1116 and 3083), which the search holds four and eight to a thread
    ("loop50", "sizes", "loop50", "en-us", "goforward.raw", 0),
    ("loop110", "sizes", "loop110", "en-us", "goforward.raw", 0),
)
MANDATORY_GROUPS = ("goforward", "loop", "nulls", "sil", "nomatch", "fr", "truncations")
GROUPS = MANDATORY_GROUPS + ("sizes",)


def fsg_path(grammar):
    return os.path.join(FSG_DIR, grammar + ".fsg")


def pcm(recording, samples):
    x = np.fromfile(os.path.join(GOLD, recording), dtype="<i2")
    return x[:samples] if samples else x


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)


def parse_fsg(path):
    """(name, n_states, start, final, [(from, to, prob, word or None)]) of a .fsg file written
    with the long keywords, one item per line (what the fixtures under tests/golden/fsg/ use)"""
    name = n = start = final = None
    trans = []
    with open(path, encoding="utf-8") as f:
        for line in f:
            t = line.split()
            if not t or line.startswith("#"):
                continue
            if t[0] == "FSG_BEGIN":
                name = t[1] if len(t) > 1 else ""
            elif t[0] == "NUM_STATES":
                n = int(t[1])
            elif t[0] == "START_STATE":
                start = int(t[1])
            elif t[0] == "FINAL_STATE":
                final = int(t[1])
            elif t[0] == "TRANSITION":
                trans.append((int(t[1]), int(t[2]), float(t[3]), t[4] if len(t) > 4 else None))
    return name, n, start, final, trans
