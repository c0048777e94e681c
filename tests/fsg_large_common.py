"""What tests/golden/make_fsg_large.py records and the large-grammar tests replay: grammars of
more than 4096 phone-tree HMMs (ssw_grammar_prepare_large), in the terms of tests/fsg_common.py."""
import json
import os

from tests import fsg_common as C

RESULTS_JSON = os.path.join(C.GOLD, "fsg_large_results.json")

# grammar -> (words, every n-th qualifying dictionary entry, states); see make_fsg_large.py
GRAMMARS = {"loop200": (200, 600, 1), "loop400": (400, 300, 1), "nulls200": (200, 600, 3)}

# (case, group, grammar, model, recording, samples (0: the whole recording))
CASES = (
    ("loop200", "large", "loop200", "en-us", "goforward.raw", 0),
    ("loop400", "large", "loop400", "en-us", "goforward.raw", 0),
    ("nulls200", "large", "nulls200", "en-us", "goforward.raw", 0),
    ("loop200_1200ms", "large_truncations", "loop200", "en-us", "goforward.raw", 19200),
    ("loop400_1200ms", "large_truncations", "loop400", "en-us", "goforward.raw", 19200),
    ("nulls200_1200ms", "large_truncations", "nulls200", "en-us", "goforward.raw", 19200),
)

# the reference's phone-tree HMMs per grammar, and (hypothesis, score) per case
HMMS = {"loop200": 5613, "loop400": 11818, "nulls200": 5617}
TRUTH = {
    "loop200": ("go forward ten meters", -8990), "loop200_1200ms": ("go forward", -3827),
    "loop400": ("go forward ten meters", -9162), "loop400_1200ms": ("go forward", -3913),
    "nulls200": ("go forward ten meters", -9166), "nulls200_1200ms": ("go forward", -3915),
}


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)
