"""Times recognition in the reference's DEFAULT configuration (compallsen = no) against grammars
beyond one workgroup (ssw_grammar_prepare_large_active: grammar_search_big_kernel<1024, EXPORT>
under the rounds of speculation and proof) and writes profiles/grammar_large_active_bench.json.

loop200 and loop400 (tests/golden/fsg/, 5613 and 11818 phone-tree HMMs), each at 1, 16 and 256
copies of the committed recording (tests/golden/goforward.raw, 278 feature rows; front end and
features on the GPU, not timed).  Per grammar and size, alternating and repeated:

    yes         ssw_recognize_batch on the flagged plan: all senones scored, one search -- the
                path a plan without the flag takes, the yardstick
    active      ssw_recognize_batch_active: scoring included, every round

with the rounds every utterance took (maximum and mean), the history groups of the call and
`ratio` = active / yes medians.  Each figure is the host clock around one synchronous call, the
median and the spread of --reps calls after --warmup calls.  The expectation to hold the active
figure against is scoring + (1 + rounds) x (plan + listed scoring + one search); SSW_ALIGN_TIMING=1
makes the library print each round's split on stderr.  The file is rewritten after every size, so
a run that is cut short leaves what it measured.  Needs a GPU.

    python tools/bench_grammar_large_active.py [--sizes 1,16,256] [--reps 5] [--warmup 1] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1,16,256")
    ap.add_argument("--grammars", default="loop200,loop400")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grammar_large_active_bench.json"))
    a = ap.parse_args()

    import torch

    import soundswallower_amd as ssw
    from tests import fsg_common as G

    if not torch.cuda.is_available():
        sys.exit("bench_grammar_large_active: no GPU; nothing is measured without one")
    sizes = [int(x) for x in a.sizes.split(",")]
    names = a.grammars.split(",")
    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    cep, _ = m.fe_batch(G.pcm("goforward.raw", 0))
    feats = np.ascontiguousarray(m.feat_batch(cep), np.float32)
    T = len(feats)
    d = torch.from_numpy(np.ascontiguousarray(np.tile(feats, (max(sizes), 1)))).cuda()
    plans = {g: lex.grammar_plan(ssw.Fsg.read(m, lex, G.fsg_path(g)), max_hmms=30000, active=True)
             for g in names}
    offs = {n: (np.arange(n + 1) * T).astype(np.int32) for n in sizes}
    out = {
        "what": "ssw_recognize_batch_active (compallsen = no) / ssw_recognize_batch (compallsen = "
                "yes) from feature rows on plans made by ssw_grammar_prepare_large_active, host "
                "clock around one synchronous call, ms; measured on the GPU named below",
        "device": torch.cuda.get_device_name(0),
        "frames_per_utterance": T, "reps": a.reps, "warmup": a.warmup,
        "hmms": {g: plans[g].hmms() for g in names},
        "hyp_and_score": {}, "history_groups": {}, "ms": {}, "rounds": {}, "ratio": {},
    }
    last = {}

    def run_yes(g, n):
        r = ssw.recognize_batch(m, lex, d, offs[n], plans[g])
        last["yes"] = (r.hyp(n - 1), r.score(n - 1))
        r.free()

    def run_active(g, n):
        r, rounds = ssw.recognize_batch_active(m, lex, d, offs[n], plans[g])
        last["active"] = (r.hyp(n - 1), r.score(n - 1))
        last["rounds"] = rounds
        r.free()

    calls = {"yes": run_yes, "active": run_active}
    for n in sizes:
        for g in names:
            times = {k: [] for k in calls}
            for i in range(a.warmup + a.reps):
                for k, fn in calls.items():      # alternating: both share whatever the box does
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fn(g, n)
                    dt = (time.perf_counter() - t0) * 1e3
                    if i >= a.warmup:
                        times[k].append(dt)
            rounds = last["rounds"]
            out["ms"].setdefault(g, {})[str(n)] = {
                k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                    "max": round(max(v), 4)} for k, v in times.items()}
            out["rounds"].setdefault(g, {})[str(n)] = {
                "max": int(rounds.max()), "mean": round(float(rounds.mean()), 3)}
            out["history_groups"].setdefault(g, {})[str(n)] = plans[g].history_groups(offs[n])
            out["ratio"].setdefault(g, {})[str(n)] = round(
                statistics.median(times["active"]) / statistics.median(times["yes"]), 3)
            out["hyp_and_score"][g] = {"active": last["active"], "yes": last["yes"]}
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")
            print(g, n, json.dumps(out["ms"][g][str(n)]), json.dumps(out["rounds"][g][str(n)]),
                  flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
