#!/usr/bin/env python3
"""Times a continuous-density model in the reference's default configuration (compallsen = no)
beside the whole-row route, on one build and one card: align_text_batch_active next to
align_text_batch, for C3 and for a 32-density C1 (tests/cont_common.py), at 256 utterances of
1000 frames (goforward's feature rows three times over and the first 166 again, with the text to
match).  Wall time of each call, the kernel events of ssw_set_kernel_timing around the scoring
launches, the mean number of listed senones per frame (from the proven sets
ssw_recognize_batch_active hands back for the chain grammar of the same text, on 16 of the
utterances) and the rounds.  One more figure: cont_listed_kernel on a batch in which EVERY senone
is listed, beside cont_score_kernel on the same frames -- the listed kernel is not built for that
case and is expected to be slower.

    python tools/bench_cont_active.py [--utts 256] [--reps 3] [--out profiles/cont_active.json]

No pass criterion rests on these numbers."""
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
from tests import cont_common as CC  # noqa: E402

TEXT = ("go forward ten meters " * 3 + "go forward ten").split()
FRAMES = 1000


def utterance():
    f = CC.features()
    return np.concatenate([f, f, f, f[:FRAMES - 3 * len(f)]]).astype(np.float32)


def timed(fn, reps):
    best = None
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best, out


def bench_model(name, d, n_utts, reps):
    m = ssw.Model(**CC.model_paths(d), active=True)
    lex = ssw.Lexicon(m, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    x = np.tile(utterance(), (n_utts, 1))
    off = (np.arange(n_utts + 1) * FRAMES).astype(np.int32)
    texts = [TEXT] * n_utts
    d_x = m.to_device(x)
    rec = {"model": name, "n_sen": m.n_sen, "n_density": m.n_density, "veclen": list(m.veclen),
           "topn": m.topn, "utterances": n_utts, "frames": FRAMES}
    m.set_kernel_timing(True)

    def whole():
        a = ssw.align_text_batch(m, lex, d_x, off, texts)
        ok = sum(a.status(u) == 0 for u in range(n_utts))
        a.free()
        return ok

    def active():
        a = ssw.align_text_batch_active(m, lex, d_x, off, texts)
        ok = sum(a.status(u) == 0 for u in range(n_utts))
        a.free()
        return ok

    whole(), active()                                    # (workspaces, plans)
    rec["align_text_batch_ms"], rec["aligned_whole"] = timed(whole, reps)
    rec["align_text_batch_score_kernels_ms"] = list(m.kernel_timing())
    rec["align_text_batch_active_ms"], rec["aligned_active"] = timed(active, reps)
    # (the call's last scoring launch: the second pass's listed rows)
    rec["align_text_batch_active_last_listed_launch_ms"] = sum(m.kernel_timing())
    st0 = m.first_pass_active_stats()
    _, rounds = lex.first_pass_active(d_x, off, texts)
    st1 = m.first_pass_active_stats()
    rec["rounds_max"], rec["rounds_mean"] = int(rounds.max()), float(rounds.mean())
    rec["utterances_beyond_one_round"] = st1[3] - st0[3]
    # the proven listed sets of 16 utterances, through the chain grammar of the text
    k = min(16, n_utts)
    chain = ssw.Fsg.create(m, lex, "chain", 0, len(TEXT), [(i, i + 1, 1.0, w) for i, w in enumerate(TEXT)])
    r, _, listed = ssw.recognize_batch_active(m, lex, d_x, off[:k + 1], lex.grammar_plan(chain),
                                              want_listed=True)
    r.free()
    bits = np.unpackbits(np.ascontiguousarray(listed).view(np.uint8), axis=-1)
    rec["listed_senones_per_frame_mean"] = float(bits.sum() / (k * FRAMES))
    # every senone listed, beside the whole-row kernel, on 4096 frames
    n = min(4096, len(x))
    out = m.device_malloc(n * m.n_sen * 2)
    every = np.full((n, (m.n_sen + 31) // 32), 0xFFFFFFFF, np.uint32)

    def score_whole():
        m.score_batch_device(d_x, n, [0, n], out)
        m._L.ssw_device_synchronize()
        return sum(m.kernel_timing())

    def score_listed():
        assert m._L.ssw_debug_cont_score_listed(m._m, d_x, n, every.ctypes.data, 0, out, None) == 0
        m._L.ssw_device_synchronize()
        return sum(m.kernel_timing())

    score_whole(), score_listed()
    rec["every_senone_listed"] = {"frames": n,
                                  "cont_score_kernel_ms": min(score_whole() for _ in range(reps)),
                                  "cont_listed_kernel_ms": min(score_listed() for _ in range(reps))}
    m.device_free(out)
    m.device_free(d_x)
    m.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cont_active.json"))
    args = ap.parse_args()
    res = []
    with tempfile.TemporaryDirectory() as tmp:
        res.append(bench_model("C3", CC.model_c3_dir(os.path.join(tmp, "C3")), args.utts, args.reps))
        res.append(bench_model("C1-32", CC.model_c1_dir(os.path.join(tmp, "C1"), k=32, n_density=32),
                               args.utts, args.reps))
    for r in res:
        print(json.dumps(r))
    with open(args.out, "w", encoding="utf-8") as f:
        json.dump({"tool": "tools/bench_cont_active.py", "results": res}, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
