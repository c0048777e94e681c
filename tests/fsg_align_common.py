"""What tests/golden/make_fsg_align.py records and the recognise-and-align tests replay: the
reference library recognising a recording against a grammar and then aligning what it recognised
(decoder_result_json at align_level 1 and 2, decoder_alignment), in both of its configurations
(compallsen = yes, and no: its default).

A case is (name, kind, grammar, model, recording, samples); kind is "fsg" (tests/golden/fsg/),
"large" (the same directory, planned with max_hmms) or "jsgf" (tests/golden/jsgf/); model is a
directory under soundswallower_amd/model/, "cb41" (the semi-continuous model of tests/sc_common)
or "C3" (the continuous model tests/cont_common builds).  A record's key is name + "/" + config."""
import json
import os

from tests import fsg_common as C
from tests import fsg_large_common as LC
from tests import jsgf_common as J

RESULTS_JSON = os.path.join(C.GOLD, "fsg_align_results.json")
CONFIGS = ("yes", "no")

CASES = tuple((n, "fsg", g, m, r, s) for (n, _, g, m, r, s) in C.CASES) + tuple(
    (n, "large", g, m, r, s) for (n, _, g, m, r, s) in LC.CASES if s == 0) + (
    ("turtle", "jsgf", "turtle", "en-us", "goforward.raw", 0),
    ("sc_goforward", "fsg", "goforward", "cb41", "goforward.raw", 0),
    ("cont_goforward", "fsg", "goforward", "C3", "goforward.raw", 0),
    ("cont_loop", "fsg", "loop", "C3", "goforward.raw", 0),
    ("cont_nulls", "fsg", "nulls", "C3", "goforward.raw", 0),
)
MAX_HMMS = 30000  # the plan of a "large" case

# what the reference was seen to do, in both configurations, before the fixture was made: the make
# script asserts it, so that the fixture pins alignments and not their absence
ALIGNED = ("goforward", "loop", "nulls", "sil", "loop110", "loop400", "nulls200")
NO_HYP = ("nomatch", "goforward_1200ms", "loop_410")


def configs(case):
    """a continuous model is recorded (and served) over whole rows only"""
    return ("yes",) if case[3] == "C3" else CONFIGS


def keys():
    return [c[0] + "/" + cfg for c in CASES for cfg in configs(c)]


def case(name):
    return next(c for c in CASES if c[0] == name)


def grammar_path(c):
    return J.gram_path(c[2]) if c[1] == "jsgf" else C.fsg_path(c[2])


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)
