"""Times the grammar search (ssw_grammar_search_batch) on the GPU and writes
profiles/grammar_bench.json.

256 copies of the committed recording (tests/golden/goforward.raw, 278 frames each), scored once
(front end, features and all senones on the GPU; not timed), then, alternating and repeated:

    goforward   the search against tests/golden/fsg/goforward.fsg
    loop        the search against tests/golden/fsg/loop.fsg
    chain_fsg   the chain "go forward ten meters" as an FSG through the grammar instance
    chain_text  the same text through ssw_first_pass_batch with its graphs prepared
                (ssw_first_pass_run), the path the grammar instance is compared with

Each figure is the host clock around one call that ends in the call's own stream synchronise
(graph upload where it is not cached, launch, results back), the median and the spread of
--reps calls after --warmup calls; `ratio_chain` = chain_fsg / chain_text medians.  Needs a GPU:
there is no CPU figure, and without a device the script fails.

    python tools/bench_grammar.py [--utts 256] [--reps 30] [--warmup 5] [--out FILE]

With --active it times, instead, recognition in the reference's DEFAULT configuration
(compallsen = no) from feature rows and writes profiles/grammar_active_bench.json: the same 256
copies, every utterance against grammar 0 (goforward) or 1 (loop) of one plan in turn,

    active      ssw_recognize_batch_active: speculation and proof, scoring included
    yes         ssw_recognize_batch on the same features and plan: all senones scored, one search

alternating, with the rounds every utterance took and their histogram; `ratio` = active / yes
medians.

    python tools/bench_grammar.py --active [--utts 256] [--reps 10] [--warmup 2] [--out FILE]

With --large it times grammars beyond one workgroup (ssw_grammar_prepare_large: node state and
exchange arrays in an HBM workspace) and writes profiles/grammar_large_bench.json: loop200 and
loop400 (tests/golden/fsg/, 5613 and 11818 phone-tree HMMs) and, as the yardstick, loop110 (3083,
the one-workgroup kernel with eight HMMs per thread), each at 1, 16 and 256 copies of the
recording; per figure the number of history groups the call is searched in, and `ratio_400_200`.

    python tools/bench_grammar.py --large [--reps 10] [--warmup 2] [--out FILE]

With --recognize-align it times phone and state times for recognised speech, from feature rows,
on the goforward plan and writes profiles/recognize_align_bench.json: the same 256 copies,

    goforward         ssw_recognize_batch: all senones scored, one search (words only)
    recognize_align   ssw_recognize_align_batch: the same, then decoder_alignment of the result
    align_text        ssw_align_text_batch of the words "go forward ten meters": scoring, first
                      pass over the text's graphs, decoder_alignment

and the three in the default configuration (compallsen = no: ssw_recognize_batch_active,
ssw_recognize_align_batch_active, ssw_align_text_batch_active) as `*_active`; alternating, the
median of --reps calls after --warmup.

    python tools/bench_grammar.py --recognize-align [--utts 256] [--reps 10] [--warmup 2] [--out FILE]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def active(a):
    import torch

    import soundswallower_amd as ssw
    from tests import fsg_common as G

    if not torch.cuda.is_available():
        sys.exit("bench_grammar: no GPU; nothing is measured without one")
    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    cep, _ = m.fe_batch(G.pcm("goforward.raw", 0))
    feats = np.ascontiguousarray(m.feat_batch(cep), np.float32)
    T, n = len(feats), a.utts
    d = torch.from_numpy(np.ascontiguousarray(np.tile(feats, (n, 1)))).cuda()
    off = (np.arange(n + 1) * T).astype(np.int32)
    names = ["goforward", "loop"]
    plan = lex.grammar_plan([ssw.Fsg.read(m, lex, G.fsg_path(g)) for g in names])
    which = (np.arange(n) % 2).astype(np.int32)
    last = {}

    def run_active():
        r, rounds = ssw.recognize_batch_active(m, lex, d, off, plan, which)
        last["active"] = (r.hyp(0), r.score(0), r.hyp(1), r.score(1))
        last["rounds"] = rounds
        r.free()

    def run_yes():
        r = ssw.recognize_batch(m, lex, d, off, plan, which)
        last["yes"] = (r.hyp(0), r.score(0), r.hyp(1), r.score(1))
        r.free()

    calls = {"active": run_active, "yes": run_yes}
    times = {k: [] for k in calls}
    for i in range(a.warmup + a.reps):
        for k, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                times[k].append(dt)
    rounds = last["rounds"]
    out = {
        "what": "ssw_recognize_batch_active (compallsen = no) / ssw_recognize_batch (compallsen = "
                "yes) from feature rows, host clock around one synchronous call, ms; measured on "
                "the GPU named below",
        "device": torch.cuda.get_device_name(0),
        "utterances": n, "frames_per_utterance": T, "reps": a.reps, "warmup": a.warmup,
        "grammars": names, "hmms": [plan.hmms(i) for i in range(len(names))],
        "hyp_and_score": {"active": last["active"], "yes": last["yes"]},
        "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                   "max": round(max(v), 4)} for k, v in times.items()},
        "rounds_per_utterance": [int(x) for x in rounds],
        "rounds_histogram": np.bincount(rounds, minlength=2).tolist(),
        "rounds_of_the_call": int(m.grammar_active_stats()[2]),
    }
    out["ratio"] = round(out["ms"]["active"]["median"] / out["ms"]["yes"]["median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def recognize_align(a):
    import torch

    import soundswallower_amd as ssw
    from tests import fsg_common as G

    if not torch.cuda.is_available():
        sys.exit("bench_grammar: no GPU; nothing is measured without one")
    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    cep, _ = m.fe_batch(G.pcm("goforward.raw", 0))
    feats = np.ascontiguousarray(m.feat_batch(cep), np.float32)
    T, n = len(feats), a.utts
    d = torch.from_numpy(np.ascontiguousarray(np.tile(feats, (n, 1)))).cuda()
    off = (np.arange(n + 1) * T).astype(np.int32)
    plan = lex.grammar_plan(ssw.Fsg.read(m, lex, G.fsg_path("goforward")))
    texts = ssw.Texts(["go forward ten meters".split()] * n)
    last = {}

    def free(*sets):
        for s in sets:
            s.free()

    def run_goforward():
        r = ssw.recognize_batch(m, lex, d, off, plan)
        last["goforward"] = (r.hyp(n - 1), r.score(n - 1))
        free(r)

    def run_recognize_align():
        r, al = ssw.recognize_align_batch(m, lex, d, off, plan)
        last["recognize_align"] = (r.hyp(n - 1), r.score(n - 1), al.status(n - 1))
        free(r, al)

    def run_align_text():
        al = ssw.align_text_batch(m, lex, d, off, texts)
        last["align_text"] = al.status(n - 1)
        free(al)

    def run_goforward_active():
        r, _ = ssw.recognize_batch_active(m, lex, d, off, plan)
        last["goforward_active"] = (r.hyp(n - 1), r.score(n - 1))
        free(r)

    def run_recognize_align_active():
        r, al, _ = ssw.recognize_align_batch_active(m, lex, d, off, plan)
        last["recognize_align_active"] = (r.hyp(n - 1), r.score(n - 1), al.status(n - 1))
        free(r, al)

    def run_align_text_active():
        al = ssw.align_text_batch_active(m, lex, d, off, texts)
        last["align_text_active"] = al.status(n - 1)
        free(al)

    calls = {"goforward": run_goforward, "recognize_align": run_recognize_align,
             "align_text": run_align_text, "goforward_active": run_goforward_active,
             "recognize_align_active": run_recognize_align_active,
             "align_text_active": run_align_text_active}
    times = {k: [] for k in calls}
    for i in range(a.warmup + a.reps):
        for k, fn in calls.items():          # alternating: the calls share whatever the box does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                times[k].append(dt)
    out = {
        "what": "recognition with phone and state times (ssw_recognize_align_batch[_active]) next "
                "to recognition alone (ssw_recognize_batch[_active]) and to text alignment of the "
                "same words (ssw_align_text_batch[_active]), from feature rows, host clock around "
                "one synchronous call, ms; measured on the GPU named below",
        "device": torch.cuda.get_device_name(0),
        "utterances": n, "frames_per_utterance": T, "reps": a.reps, "warmup": a.warmup,
        "hmms": plan.hmms(), "results_of_the_last_utterance": last,
        "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                   "max": round(max(v), 4)} for k, v in times.items()},
    }
    med = {k: out["ms"][k]["median"] for k in times}
    out["ratio_to_goforward"] = round(med["recognize_align"] / med["goforward"], 3)
    out["ratio_to_align_text"] = round(med["recognize_align"] / med["align_text"], 3)
    out["ratio_to_goforward_active"] = round(med["recognize_align_active"] / med["goforward_active"], 3)
    out["ratio_to_align_text_active"] = round(med["recognize_align_active"] / med["align_text_active"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def large(a):
    import torch

    import soundswallower_amd as ssw
    from tests import fsg_common as G

    if not torch.cuda.is_available():
        sys.exit("bench_grammar: no GPU; nothing is measured without one")
    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    cep, _ = m.fe_batch(G.pcm("goforward.raw", 0))
    scr = m.score_batch(m.feat_batch(cep))
    T, sizes = len(scr), (1, 16, 256)
    d = torch.from_numpy(np.ascontiguousarray(np.tile(scr, (max(sizes), 1)))).cuda()
    names = ["loop110", "loop200", "loop400"]
    plans = {g: lex.grammar_plan(ssw.Fsg.read(m, lex, G.fsg_path(g)),
                                 max_hmms=None if g == "loop110" else 30000) for g in names}
    offs = {n: (np.arange(n + 1) * T).astype(np.int32) for n in sizes}
    last = {}

    def run(g, n):
        r = ssw.grammar_search_batch(m, lex, d, offs[n], plans[g])
        last[g] = (r.hyp(n - 1), r.score(n - 1))
        r.free()

    times = {(g, n): [] for n in sizes for g in names}
    for n in sizes:
        for i in range(a.warmup + a.reps):
            for g in names:                  # alternating: the grammars share whatever the box does
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(g, n)
                dt = (time.perf_counter() - t0) * 1e3
                if i >= a.warmup:
                    times[(g, n)].append(dt)
    out = {
        "what": "ssw_grammar_search_batch, host clock around one synchronous call, ms; loop200 and "
                "loop400 on grammar_search_big_kernel (ssw_grammar_prepare_large), loop110 on "
                "grammar_search_kernel<8, 512>; measured on the GPU named below",
        "device": torch.cuda.get_device_name(0),
        "frames_per_utterance": T, "reps": a.reps, "warmup": a.warmup,
        "hmms": {g: plans[g].hmms() for g in names},
        "hyp_and_score": last,
        "history_groups": {g: {str(n): plans[g].history_groups(offs[n]) for n in sizes}
                           for g in names},
        "ms": {g: {str(n): {"median": round(statistics.median(times[(g, n)]), 4),
                            "min": round(min(times[(g, n)]), 4),
                            "max": round(max(times[(g, n)]), 4)} for n in sizes} for g in names},
        "reference": "about 200 ms of one CPU core per utterance for these grammars, model load "
                     "included (an upper bound)",
    }
    out["ms_per_utterance"] = {g: {str(n): round(out["ms"][g][str(n)]["median"] / n, 4)
                                   for n in sizes} for g in names}
    out["ratio_400_200"] = {str(n): round(out["ms"]["loop400"][str(n)]["median"]
                                          / out["ms"]["loop200"][str(n)]["median"], 3)
                            for n in sizes}
    out["hmm_ratio_400_200"] = round(out["hmms"]["loop400"] / out["hmms"]["loop200"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--active", action="store_true",
                    help="time ssw_recognize_batch_active next to ssw_recognize_batch instead")
    ap.add_argument("--large", action="store_true",
                    help="time grammars beyond one workgroup (ssw_grammar_prepare_large) instead")
    ap.add_argument("--recognize-align", action="store_true", dest="recognize_align",
                    help="time ssw_recognize_align_batch next to ssw_recognize_batch and "
                         "ssw_align_text_batch instead")
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "recognize_align_bench.json" if a.recognize_align
                             else "grammar_large_bench.json" if a.large
                             else "grammar_active_bench.json" if a.active
                             else "grammar_bench.json")
    if a.recognize_align:
        return recognize_align(a)
    if a.active:
        return active(a)
    if a.large:
        return large(a)

    import torch

    import soundswallower_amd as ssw
    from soundswallower_amd import _lib
    from soundswallower_amd.api import WORD_SEG_DTYPE, _ptr
    from tests import fsg_common as G

    if not torch.cuda.is_available():
        sys.exit("bench_grammar: no GPU; nothing is measured without one")
    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    cep, _ = m.fe_batch(G.pcm("goforward.raw", 0))
    scr = m.score_batch(m.feat_batch(cep))
    T, n = len(scr), a.utts
    d = torch.from_numpy(np.ascontiguousarray(np.tile(scr, (n, 1)))).cuda()
    off = (np.arange(n + 1) * T).astype(np.int32)
    words = "go forward ten meters".split()

    plans = {
        "goforward": lex.grammar_plan(ssw.Fsg.read(m, lex, G.fsg_path("goforward"))),
        "loop": lex.grammar_plan(ssw.Fsg.read(m, lex, G.fsg_path("loop"))),
        "chain_fsg": lex.grammar_plan(ssw.Fsg.create(
            m, lex, "chain", 0, len(words), [(i, i + 1, 1.0, w) for i, w in enumerate(words)])),
    }
    text_plan = ssw.FirstPassPlan(m, lex, [words] * n)
    L = _lib.lib()
    max_seg = 4 * len(words) + 8
    n_seg = np.zeros(n, np.int32)
    seg = np.zeros((n, max_seg), WORD_SEG_DTYPE)

    def run_text():
        rc = L.ssw_first_pass_run(m._m, text_plan._p, _ptr(d), int(off[-1]), _ptr(off), max_seg,
                                  _ptr(n_seg), _ptr(seg), None)
        assert rc == 0, _lib.last_error()

    def run_fsg(name):
        r = ssw.grammar_search_batch(m, lex, d, off, plans[name])
        r.free()

    calls = {"goforward": lambda: run_fsg("goforward"), "loop": lambda: run_fsg("loop"),
             "chain_fsg": lambda: run_fsg("chain_fsg"), "chain_text": run_text}
    # the results the timed calls compute, once, for the record
    r = ssw.grammar_search_batch(m, lex, d, off, plans["chain_fsg"])
    run_text()
    total, got = 0, []
    for w, sf, ef, ascr, lscr in r.segments(n - 1):
        total += ascr + lscr
        got.append((w, sf, ef - sf + 1, total))
    want = [(lex.word(int(s["wid"])), int(s["start"]), int(s["duration"]), int(s["score"]))
            for s in seg[n - 1, :n_seg[n - 1]]]
    same = got == want
    hyp = {k: ssw.grammar_search_batch(m, lex, d, off, plans[k]).hyp(0) for k in plans}

    times = {k: [] for k in calls}
    for i in range(a.warmup + a.reps):
        for k, fn in calls.items():          # alternating: the versions share whatever the box does
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= a.warmup:
                times[k].append(dt)
    out = {
        "what": "ssw_grammar_search_batch / ssw_first_pass_run, host clock around one synchronous "
                "call, ms; measured on the GPU named below",
        "device": torch.cuda.get_device_name(0),
        "utterances": n, "frames_per_utterance": T, "reps": a.reps, "warmup": a.warmup,
        "hmms": {k: plans[k].hmms() for k in plans},
        "hyp": hyp,
        "chain_fsg_equals_chain_text": bool(same),
        "ms": {k: {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                   "max": round(max(v), 4)} for k, v in times.items()},
    }
    out["us_per_frame"] = {k: round(1e3 * out["ms"][k]["median"] / T, 3) for k in times}
    out["ratio_chain"] = round(out["ms"]["chain_fsg"]["median"] / out["ms"]["chain_text"]["median"], 3)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
