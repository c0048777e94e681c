#!/usr/bin/env python3
"""Timing of the s2_semi scorer (single-codebook models) beside en-us PTM scoring in one process.

Models A (en-us cut down to codebook 41: 3 streams of 13 dimensions, 128 densities) and B (streams
of 12, 24, 3 and 12 dimensions, 256 densities) are made as the tests make them
(tests/sc_common.py).  Each shape is scored `steps` times back to back over one resident batch
after a warm-up, the wall time between two device synchronisations gives frames/s, and 20 more
calls with ssw_set_kernel_timing give the milliseconds per kernel from HIP events.  The yardstick
is en-us through the PTM kernels at the same frame counts.  Prints one JSON line per shape; with
--out the lines are also written to a file (profiles/sc_bench.json).
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import soundswallower_amd as ssw  # noqa: E402
from soundswallower_amd import _lib  # noqa: E402
from soundswallower_amd.synth import read_raw_means, synth_features  # noqa: E402
from tests import sc_common as S  # noqa: E402


def measure(m, feats, utts, frames, steps, warmup, name):
    L = _lib.lib()
    n = utts * frames
    assert feats.shape[0] >= n
    off = (np.arange(utts + 1) * frames).astype(np.int32)
    d_feats = m.to_device(feats[:n])
    d_out = L.ssw_device_malloc(n * m.n_sen * 2)
    scorer = m.pick_scorer()

    def step():
        m.score_batch_device(d_feats, n, off, d_out, scorer=scorer)

    t_spin = time.perf_counter()
    while time.perf_counter() - t_spin < 0.3:
        for _ in range(10):
            step()
        L.ssw_device_synchronize()
    for _ in range(warmup):
        step()
    L.ssw_device_synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    L.ssw_device_synchronize()
    dt = time.perf_counter() - t0
    m.set_kernel_timing(True)
    k = np.zeros(3)
    ms = np.zeros(3, np.float32)
    got = 0
    for _ in range(20):
        step()
        ms[:] = 0
        got = L.ssw_get_kernel_timing(m._m, ms.ctypes.data, 3)
        k += ms
    k /= 20
    m.set_kernel_timing(False)
    m.device_free(d_feats)
    L.ssw_device_free(d_out)
    line = {"model": name, "scorer": {0: "ptm", 1: "ms", 2: "s2_semi"}[scorer], "utts": utts,
            "frames_per_utt": frames, "frames": n, "steps": steps,
            "frames_per_s": n * steps / dt, "ms_per_call": dt / steps * 1e3,
            "n_feat": m.n_feat, "n_density": m.n_density, "veclen": m.veclen, "n_sen": m.n_sen}
    if got == 3:
        line.update(density_kernel_ms=float(k[0] - k[2]), chain_kernel_ms=float(k[2]),
                    senone_kernel_ms=float(k[1]))
    elif got == 2:
        line.update(topn_kernels_ms=float(k[0]), senone_kernel_ms=float(k[1]))
    else:
        line.update(call_ms=float(k[0]))
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    _lib.build()
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        en = ssw.Model(ssw.model_dir("en-us"))
        f_en = np.concatenate([synth_features(read_raw_means(ssw.model_dir("en-us")), 256, 4242 + u)
                               for u in range(16)])
        ma = ssw.Model(S.model_a_dir(os.path.join(tmp, "A")))
        means_a = np.stack([s for s in S.read_gauss(os.path.join(S.MODEL_A, "means"))[2]], axis=1)
        f_a = np.concatenate([synth_features(means_a, 256, 4242 + u) for u in range(16)])
        mb = ssw.Model(S.model_b_dir(os.path.join(tmp, "B")))
        f_b = S.model_b_features(S.model_b_tables()[0], 4096)
        for name, m, f, utts, frames in (("en-us", en, f_en, 16, 256), ("A", ma, f_a, 16, 256),
                                         ("B", mb, f_b, 16, 256), ("en-us", en, f_en, 1, 4096),
                                         ("A", ma, f_a, 1, 4096)):
            lines.append(measure(m, f, utts, frames, a.steps, a.warmup, name))
            print(json.dumps(lines[-1]), flush=True)
    if a.out:
        with open(a.out, "w", encoding="utf-8") as fh:
            for line in lines:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
