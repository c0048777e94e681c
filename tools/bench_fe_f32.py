"""The front end on int16 and on float32 samples (ssw_fe_batch_ex, ssw_fe_batch_f32): the same
16 kHz batch through both entry points.

    python tools/bench_fe_f32.py [--utts 512] [--frames 1000] [--reps 3] [--out profiles/fe_f32.json]

Prints (and with --out writes) one JSON object: per entry point `reps` repeats, each the whole
call in ms (device samples in, device cepstra out) and its split over the three kernels
(spectrum, noise, cepstrum) from HIP events (ssw_fe_kernel_timing), with the spread of the
repeats.  The float audio is the int16 audio / 32768, so both paths compute the same cepstra,
which is checked.  On a build without the float32 entry point (an older library loaded through
SSW_AMD_LIB) only the int16 path is timed: the figure of the commit before it."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def measure(m, torch, call, reps):
    call()                                    # warm-up (tables, workspaces)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        t = time.perf_counter() - t0
        m.set_kernel_timing(True)
        call()
        ms = m.fe_kernel_timing()
        m.set_kernel_timing(False)
        out.append({"call_ms": round(t * 1e3, 3), "spectrum_ms": round(ms[0], 3),
                    "noise_ms": round(ms[1], 3), "cep_ms": round(ms[2], 3)})
    return out


def spread(runs, key):
    v = [r[key] for r in runs]
    return {"min": min(v), "median": float(np.median(v)), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=512)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--model-dir", help="the en-us model (default: the package's own)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch

    import soundswallower_amd as ssw
    from bench_fe import audio, samples_for
    from soundswallower_amd import _lib

    m = ssw.Model(a.model_dir or ssw.model_dir("en-us"))
    ns = samples_for(a.frames)
    pcm = audio(a.utts, ns)
    off = np.arange(a.utts + 1, dtype=np.int64) * ns
    n_frames = int(ssw.fe_frame_counts(np.diff(off)).sum())
    res = {"metric": "front end, int16 against float32 samples",
           "workload": f"{a.utts} x {a.frames} frames of 16 kHz audio, en-us feat_params.json",
           "frames": n_frames, "reps": a.reps}
    d16 = torch.from_numpy(pcm).cuda()
    c16 = torch.empty((n_frames, 13), dtype=torch.float32, device="cuda")
    res["int16"] = measure(m, torch, lambda: m.fe_batch_rates_device(d16, off, 16000, c16), a.reps)
    if hasattr(_lib.lib(), "ssw_fe_batch_f32"):
        d32 = torch.from_numpy(pcm.astype(np.float32) / np.float32(32768)).cuda()
        c32 = torch.empty((n_frames, 13), dtype=torch.float32, device="cuda")
        res["float32"] = measure(m, torch, lambda: m.fe_batch_f32_device(d32, off, 16000, c32),
                                 a.reps)
        res["same_cepstra"] = bool(torch.equal(c16.view(torch.int32), c32.view(torch.int32)))
    for k in ("int16", "float32"):
        if k in res:
            res[k + "_spread"] = {q: spread(res[k], q) for q in ("call_ms", "spectrum_ms")}
    if "float32" in res:
        lo, hi = res["int16_spread"]["spectrum_ms"]["min"], res["int16_spread"]["spectrum_ms"]["max"]
        med = res["float32_spread"]["spectrum_ms"]["median"]
        res["float32_spectrum_within_int16_spread"] = bool(lo <= med <= hi)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
