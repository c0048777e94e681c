#!/usr/bin/env python3
"""Timing of the ms scorer on continuous-density models (one codebook per senone) beside en-us
PTM scoring in one process.

The models are made as the tests make them (tests/cont_common.py): C3 (5126 codebooks, 3 streams of
13 dimensions, 8 densities), C1 (one stream of 39, 6 densities) and C1-32 (the same shape with 32
densities, cut from en-us in the same way).  Each is scored `steps` times back to back over one
resident batch of en-us-like features after a warm-up (tools/bench_sc.py: measure), at 16 x 256
frames and at one utterance of 4096; the wall time between two device synchronisations gives
ms per call, 20 more calls with ssw_set_kernel_timing the split into cont_score_kernel and
cont_norm_kernel.  en-us through the PTM kernels on the same batch is recorded beside each.
Prints one JSON line per measurement; --out writes them to a file (profiles/cont_bench.json),
--headline FILE adds the lines of FILE (the headline benchmark's runs at this commit and at its
parent, as the job that ran them wrote them) under "headline".
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import soundswallower_amd as ssw  # noqa: E402
from bench_sc import measure  # noqa: E402
from soundswallower_amd import _lib  # noqa: E402
from soundswallower_amd.synth import read_raw_means, synth_features  # noqa: E402
from tests import cont_common as CC  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--headline", default=None)
    a = ap.parse_args()
    _lib.build()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        en = ssw.Model(ssw.model_dir("en-us"))
        feats = np.concatenate([synth_features(read_raw_means(ssw.model_dir("en-us")), 256, 4242 + u)
                                for u in range(16)])
        models = [("en-us", en),
                  ("C3", ssw.Model(**CC.model_paths(CC.model_c3_dir(os.path.join(tmp, "C3"))))),
                  ("C1", ssw.Model(**CC.model_paths(CC.model_c1_dir(os.path.join(tmp, "C1"))))),
                  ("C1-32", ssw.Model(**CC.model_paths(CC.model_c1_dir(os.path.join(tmp, "C1-32"),
                                                                       32, 32))))]
        for utts, frames in ((16, 256), (1, 4096)):
            for name, m in models:
                line = measure(m, feats, utts, frames, a.steps, a.warmup, name)
                if m.continuous:
                    line["topn"] = m.topn
                    line["score_kernel_ms"] = line.pop("topn_kernels_ms")
                    line["norm_kernel_ms"] = line.pop("senone_kernel_ms")
                lines.append(line)
                print(json.dumps(line), flush=True)
    if a.headline:
        with open(a.headline, encoding="utf-8") as fh:
            lines.append({"headline": [json.loads(s) for s in fh if s.strip()]})
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
