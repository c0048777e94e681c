#!/usr/bin/env python3
"""Writes tests/golden/fsg_large_default_results.json: the reference library, in its DEFAULT
configuration (compallsen = no), recognising goforward.raw against the large grammars under
tests/golden/fsg/ (loop200, loop400, nulls200: more than 4096 phone-tree HMMs each), whole and cut
to 19200 samples -- the truth that ssw_recognize_batch_active on a plan made by
ssw_grammar_prepare_large_active is tested against.

It compiles tests/harness/fsg_default_driver.c against the reference library that build() makes
in oracle/_ref/ (oracle/reference.py) and runs it once per case of tests/fsg_large_common.CASES,
with no setting but loglevel.  The records have the format of make_fsg_default.py's; the grammars
are the ones make_fsg_large.py writes, read as they are.

    python tests/golden/make_fsg_large_default.py           # rewrite the fixture
    python tests/golden/make_fsg_large_default.py --check   # rewrite nothing; exit 1 and name every
                                                            # case whose record would change
"""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from oracle import reference  # noqa: E402
from tests import fsg_large_common as CL  # noqa: E402
from tests import fsg_large_default_common as CD  # noqa: E402
import make_fsg_default  # noqa: E402


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        exe = make_fsg_default.build_driver(tmp)
        got = {case[0]: make_fsg_default.run_case(exe, case) for case in CL.CASES}
    if check:
        have = CD.results() if os.path.exists(CD.RESULTS_JSON) else {}
        bad = [k for k in sorted(set(got) | set(have)) if have.get(k) != got.get(k)]
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(CD.RESULTS_JSON, "w", encoding="utf-8") as f:
        json.dump(got, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(got)} cases, {os.path.getsize(CD.RESULTS_JSON)} bytes")


if __name__ == "__main__":
    main()
