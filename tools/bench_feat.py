#!/usr/bin/env python3
"""Timing of the dynamic-feature kernels: ssw_feat_batch (one workgroup per utterance) beside
ssw_feat_batch_ex (statistics per utterance, then frame-parallel tiles) on the same resident
cepstra.

Two batches of seeded random cepstra (13 a frame): 2048 utterances of 1000 frames (BASELINE.json
configs[4]) and one utterance of 96,000 frames (the README's 96 K-frame page, which the old kernel
gives to one workgroup).  Per batch: the plain configuration (1s_c_d_dd, batch CMN) through
ssw_feat_batch and through ssw_feat_batch_ex, then batch CMN + the 36 x 39 LDA of
tests/golden/feat_types/feature_transform, s2_4x, live CMN and batch CMN + varnorm through
ssw_feat_batch_ex.  Each call is synchronous on its stream, so the wall time of a call is the
measurement: `steps` calls after `warmup`, the median and the fastest in ms.  The plain
configuration's two outputs are compared byte for byte once.
Prints one JSON line per measurement; --out writes them to a file
(profiles/feat_types_bench.json), --headline FILE adds the lines of FILE (the headline benchmark's
runs at this commit and at its parent, as the job that ran them wrote them) under "headline".
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import soundswallower_amd as ssw  # noqa: E402
from soundswallower_amd import _lib  # noqa: E402

LDA = os.path.join(ROOT, "tests", "golden", "feat_types", "feature_transform")
CONFIGS = [
    ("plain", dict(feat="1s_c_d_dd", cmn="batch", svspec=None)),
    ("lda_36x39", dict(feat="1s_c_d_dd", cmn="batch", svspec=None, lda=LDA)),
    ("s2_4x", dict(feat="s2_4x", cmn="batch", svspec=None)),
    ("live", dict(feat="1s_c_d_dd", cmn="live", svspec=None)),
    ("varnorm", dict(feat="1s_c_d_dd", cmn="batch", varnorm=True, svspec=None)),
]


def timed(call, steps, warmup):
    for _ in range(warmup):
        call()
    ms = []
    for _ in range(steps):
        t0 = time.perf_counter()
        call()
        ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(min(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--headline", default=None)
    a = ap.parse_args()
    _lib.build()
    m = ssw.Model(ssw.model_dir("en-us"))
    L = m._L
    lines = []
    for n_utts, per in ((2048, 1000), (1, 96000)):
        n = n_utts * per
        rng = np.random.default_rng(20261019)
        cep = rng.normal(0, 4, (n, 13)).astype(np.float32)
        cep[:, 0] = np.abs(cep[:, 0])
        off = (np.arange(n_utts + 1, dtype=np.int64) * per).astype(np.int32)
        d_cep = m.to_device(cep)
        d_out = m.device_malloc(n * 64 * 4)
        base = dict(utts=n_utts, frames_per_utt=per, steps=a.steps, warmup=a.warmup)

        def old():
            rv = L.ssw_feat_batch(m._m, d_cep, n, off.ctypes.data, n_utts, 13, d_out, None)
            assert rv == 0, _lib.last_error()

        med, best = timed(old, a.steps, a.warmup)
        want = np.zeros((n, 39), np.float32)
        L.ssw_memcpy_d2h(want.ctypes.data, d_out, want.nbytes)
        lines.append(dict(base, entry="ssw_feat_batch", config="plain", out_dim=39, ms=round(med, 4),
                          ms_min=round(best, 4), mframes_per_s=round(n / med / 1e3, 2)))
        print(json.dumps(lines[-1]), flush=True)
        for name, kw in CONFIGS:
            feat = m.feat(**kw)
            call = lambda: m.feat_batch_ex_device(d_cep, n, off, d_out, feat)  # noqa: E731
            med, best = timed(call, a.steps, a.warmup)
            line = dict(base, entry="ssw_feat_batch_ex", config=name, out_dim=feat.out_dim,
                        tile_frames=feat.tile_frames, ms=round(med, 4), ms_min=round(best, 4),
                        mframes_per_s=round(n / med / 1e3, 2))
            if name == "plain":
                got = np.zeros((n, 39), np.float32)
                L.ssw_memcpy_d2h(got.ctypes.data, d_out, got.nbytes)
                line["equals_ssw_feat_batch"] = got.tobytes() == want.tobytes()
            lines.append(line)
            print(json.dumps(line), flush=True)
            feat.free()
        m.device_free(d_cep)
        m.device_free(d_out)
    if a.headline:
        with open(a.headline, encoding="utf-8") as fh:
            lines.append({"headline": [json.loads(s) for s in fh if s.strip()]})
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
