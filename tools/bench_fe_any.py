"""The front end under the settings only ssw_fe_batch_any takes (csrc/ssw_k8_fe_any.inc): what
each of its paths costs beside the plain one, in one process.

    python tools/bench_fe_any.py [--utts 2048] [--frames 1000] [--reps 7] [--out profiles/fe_any.json]

At the shape of tools/bench_fe.py (utts x frames of 16 kHz PCM, en-us settings), per path: the
whole call (median, min and max of `reps` calls after a warm-up; device samples in, device rows
out) and ms per kernel from HIP events (spectrum, noise, cepstrum):
  plain_ex          ssw_fe_batch_ex
  plain_any         the same settings through ssw_fe_batch_any: the same kernels
  remove_dc_i16     int16 samples: the frame's sum by a parallel reduction
  remove_dc_f32     float32 samples x / 3: the sum in index order, one lane walking LDS
  htk, ncep26, smoothspec
and the same calls at `align-utts` x frames beside align_text_batch on that batch, the share
that DESIGN's K8 threshold (a quarter) is about.  Prints the JSON and writes it to --out.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_fe import audio, samples_for  # noqa: E402

PATHS = (("plain_any", {}, "i16"),
         ("remove_dc_i16", {"remove_dc": True}, "i16"),
         ("remove_dc_f32", {"remove_dc": True}, "f32"),
         ("htk", {"transform": "htk"}, "i16"),
         ("ncep26", {"ncep": 26}, "i16"),
         ("smoothspec", {"smoothspec": True}, "i16"))


def calls(fn, reps, torch):
    fn()                                      # warm-up (tables, workspaces)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"call_ms": round(float(np.median(ts)), 3), "min_ms": round(min(ts), 3),
            "max_ms": round(max(ts), 3)}


def kernels(m, fn):
    m.set_kernel_timing(True)
    try:
        fn()
        ms = m.fe_kernel_timing()
    finally:
        m.set_kernel_timing(False)
    return {"spectrum_ms": round(ms[0], 3), "noise_ms": round(ms[1], 3), "cep_ms": round(ms[2], 3)}


def measure(m, torch, d_i16, d_f32, off, reps, with_kernels):
    """every path over one batch: {name: times}"""
    out = {}
    rates = np.full(len(off) - 1, 16000.0)
    n_frames = int(m.fe_frame_counts_rates(np.diff(off), 16000).sum())
    d_cep = torch.empty((n_frames, 13), dtype=torch.float32, device="cuda")

    def ex():
        m.fe_batch_rates_device(d_i16, off, rates, d_cep)

    out["plain_ex"] = calls(ex, reps, torch)
    if with_kernels:
        out["plain_ex"].update(kernels(m, ex))
    for name, cfg, kind in PATHS:
        fe = m.fe(cfg)
        d_rows = torch.empty((n_frames, fe.out_dim), dtype=torch.float32, device="cuda")
        d_pcm = d_f32 if kind == "f32" else d_i16

        def run():
            m.fe_batch_any_device(d_pcm, off, rates, d_rows, fe)

        out[name] = calls(run, reps, torch)
        if with_kernels:
            out[name].update(kernels(m, run))
        out[name]["row_width"] = fe.out_dim
        del d_rows
        fe.free()
    for v in out.values():
        v["frames_per_s"] = round(n_frames / (v["call_ms"] * 1e-3))
    return out, n_frames


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--align-utts", type=int, default=256)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fe_any.json"))
    a = ap.parse_args()
    import torch

    import soundswallower_amd as ssw

    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    ns = samples_for(a.frames)
    pcm = audio(a.utts, ns)
    off = np.arange(a.utts + 1, dtype=np.int64) * ns
    d_i16 = torch.from_numpy(pcm).cuda()
    # float32 samples that are not int16 values: x / 3 (1.0 stands for 32768)
    d_f32 = d_i16.to(torch.float32) / 3 / 32768
    res = {"metric": "front end under any settings",
           "workload": f"{a.utts} x {a.frames} frames of 16 kHz PCM, en-us feat_params.json (20 "
                       "filters, remove_noise, dct, lifter 22) with one setting changed per path",
           "reps": a.reps}
    res["paths"], res["frames"] = measure(m, torch, d_i16, d_f32, off, a.reps, True)

    # ---- the same calls beside align_text_batch at align-utts x frames --------------------
    k = a.align_utts
    off_k = off[:k + 1]
    d_i16k = d_i16[:k * ns].clone()
    d_f32k = d_f32[:k * ns].clone()
    del d_i16, d_f32
    torch.cuda.empty_cache()
    small, _ = measure(m, torch, d_i16k, d_f32k, off_k, a.reps, False)
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    words = ("go forward ten meters " * (1 + a.frames // 280)).split()
    texts = ssw.Texts([words] * k)
    d_cep, fo = m.fe_batch_device(d_i16k, off_k)
    d_feats = torch.from_numpy(m.feat_batch(d_cep.cpu().numpy(), utt_off=fo)).cuda()
    box = {}

    def run_text():
        box["t"] = ssw.align_text_batch(m, lex, d_feats, fo, texts)

    t_text = calls(run_text, a.reps, torch)
    res["align"] = {"workload": f"{k} x {a.frames} frames, texts of {len(words)} words",
                    "align_text_batch": t_text,
                    "fe_call_ms": {n: v["call_ms"] for n, v in small.items()},
                    "fe_share_of_text": {n: round(v["call_ms"] / t_text["call_ms"], 4)
                                         for n, v in small.items()},
                    "threshold": 0.25}
    line = json.dumps(res)
    print(line)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
