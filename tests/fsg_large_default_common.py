"""What tests/golden/make_fsg_large_default.py records and the tests of the default configuration
(compallsen = no) on large grammars replay: the cases of tests/fsg_large_common.py, recognised by
the reference library with no setting but its log level."""
import json
import os

from tests import fsg_common as C

RESULTS_JSON = os.path.join(C.GOLD, "fsg_large_default_results.json")

# (hypothesis, score) per case in the default configuration; fsg_large_common.TRUTH has the
# compallsen = yes scores of the same cases
TRUTH = {
    "loop200": ("go forward ten meters", -7523), "loop200_1200ms": ("go forward", -2940),
    "loop400": ("go forward ten meters", -7917), "loop400_1200ms": ("go forward", -3142),
    "nulls200": ("go forward ten meters", -7680), "nulls200_1200ms": ("go forward", -3031),
}


def results():
    with open(RESULTS_JSON, encoding="utf-8") as f:
        return json.load(f)
