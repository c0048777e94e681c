"""What tests/golden/make_jsgf.py records and the JSGF tests replay: the cases (a grammar under
tests/golden/jsgf/, a model, a recording, a sample count, a -toprule) and the fixture file."""
import gzip
import json
import os

from tests import fsg_common as F

GOLD = F.GOLD
JSGF_DIR = os.path.join(GOLD, "jsgf")
RESULTS_JSON = os.path.join(GOLD, "jsgf_results.json")
# the fsg_model_write texts of every case (TEXT_KEYS), kept beside the fixture: thousands of lines
# of transitions that nobody reads but a test
TEXTS_GZ = os.path.join(GOLD, "jsgf_fsg_texts.json.gz")
TEXT_KEYS = ("fsg", "fsg_second", "fsg_search")
pcm = F.pcm

# (case, group, grammar, model, recording, samples (0: the whole recording), toprule or None)
CASES = (
    ("turtle", "turtle", "turtle", "en-us", "goforward.raw", 0, None),
    ("turtle_halt", "turtle", "turtle", "en-us", "goforward.raw", 0, "turtle.halt"),
    ("turtle_unqualified", "turtle", "turtle", "en-us", "goforward.raw", 0, "halt"),
    ("turtle_1200ms", "turtle", "turtle", "en-us", "goforward.raw", 19200, None),
    ("kleene", "kleene", "kleene", "en-us", "goforward.raw", 0, None),
    ("weights", "weights", "weights", "en-us", "goforward.raw", 0, None),
    ("recursion", "recursion", "recursion", "en-us", "goforward.raw", 0, None),
    ("tags", "tags", "tags", "en-us", "goforward.raw", 0, None),
    ("tags_quoted", "tags", "tags_quoted", "en-us", "goforward.raw", 0, None),
    ("fr", "fr", "fr", "fr-fr", "goforward_fr.raw", 0, None),
    ("pick_ab", "pick", "pick_ab", "en-us", "goforward.raw", 0, None),
    ("pick_first", "pick", "pick_first", "en-us", "goforward.raw", 0, None),
    ("pick_move", "pick", "pick_move", "en-us", "goforward.raw", 0, None),
    ("loop200", "loop200", "loop200", "en-us", "goforward.raw", 0, None),
)
GROUPS = ("turtle", "kleene", "weights", "recursion", "tags", "fr", "pick", "loop200")
# the two configurations every case is recorded in: compallsen = yes, and the reference's defaults
CONFIGS = ("yes", "default")
# searched on the GPU: everything the reference recognises but the host-only group
HOST_ONLY_GROUPS = ("pick",)
# beyond one workgroup: planned with max_hmms
LARGE = ("loop200",)


def gram_path(grammar):
    return os.path.join(JSGF_DIR, grammar + ".gram")


def case(name):
    return next(c for c in CASES if c[0] == name)


def results():
    """The fixture, case by case, with the texts of TEXTS_GZ put back beside the rest."""
    with open(RESULTS_JSON, encoding="utf-8") as f:
        got = json.load(f)
    with gzip.open(TEXTS_GZ, "rt", encoding="utf-8") as f:
        texts = json.load(f)
    assert sorted(texts) == sorted(got)
    for name, case_texts in texts.items():
        assert sorted(case_texts) == sorted(TEXT_KEYS)
        got[name].update(case_texts)
    return got


def loop200_text():
    """loop200.gram: a free loop over the word list of tests/golden/fsg/loop200.fsg, as
    public <loop> = <word>+; <word> = w1 | ... | w200;"""
    words = [t[3] for t in F.parse_fsg(F.fsg_path("loop200"))[4]]
    assert len(words) == 200
    rows = [" | ".join(words[i:i + 8]) for i in range(0, len(words), 8)]
    return ("#JSGF V1.0;\n// the word list of loop200.fsg as a JSGF closure (make_jsgf.py)\n"
            "grammar loop200;\n\npublic <loop> = <word>+;\n<word> = "
            + "\n       | ".join(rows) + ";\n")
