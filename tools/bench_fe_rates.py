"""The MFCC front end at each utterance's own sample rate (ssw_fe_batch_ex, csrc/ssw_k8_fe.inc):
what it costs at 16, 44.1 and 48 kHz and on a batch that mixes the three.

    python tools/bench_fe_rates.py [--utts 256] [--seconds 10] [--reps 5] [--out FILE]

Writes one JSON object (default profiles/fe_rates_bench.json) and prints it:
  rates       per batch (16000, 44100, 48000, mixed): utts x seconds of PCM, the call's ms
              (median of reps), ms per kernel from ssw_fe_kernel_timing (spectrum = every FFT
              size's launch, noise, cepstrum) and frames/s; device PCM in, device cepstra out
  align44100  align_audio_batch(samprate=44100) against align_text_batch on the same frames
              (the features of align_text_batch come from the front end beforehand, untimed)
en-us feat_params.json settings (20 filters, remove_noise, dct, lifter 22).  Audio: goforward,
resampled to each rate as tests/fe_rates_common.py does it, scaled, with noise, tiled.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import fe_rates_common as R  # noqa: E402


def audio(n_utts, rate, seconds, seed=7):
    go = R.resample(R.goforward(), rate)
    n = int(rate * seconds)
    rng = np.random.default_rng(seed)
    base = np.tile(go, -(-n // len(go)))[:n].astype(np.float32)
    out = np.empty((n_utts, n), np.int16)
    for u in range(n_utts):
        x = np.roll(base, int(rng.integers(0, len(go)))) * rng.uniform(0.3, 2.0)
        x += rng.normal(0, 50, n).astype(np.float32)
        out[u] = np.clip(np.round(x), -32768, 32767)
    return list(out)


def timed(fn, reps, torch):
    fn()                                      # warm-up (tables, workspaces)
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fe_rates_bench.json"))
    a = ap.parse_args()
    import torch

    import soundswallower_amd as ssw

    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    res = {"metric": "front end at each utterance's rate",
           "workload": f"{a.utts} utterances x {a.seconds:g} s, en-us feat_params.json "
                       "(20 filters, remove_noise, dct, lifter 22)", "rates": {}}
    batches = {r: ([r] * a.utts, audio(a.utts, r, a.seconds)) for r in (16000, 44100, 48000)}
    mix = [(16000, 44100, 48000)[u % 3] for u in range(a.utts)]
    batches["mixed"] = (mix, [batches[r][1][u] for u, r in enumerate(mix)])
    for name, (srs, pcms) in batches.items():
        off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
        d_pcm = torch.from_numpy(np.concatenate(pcms)).cuda()
        n_frames = int(ssw.fe_frame_counts_at(np.diff(off), srs).sum())
        d_cep = torch.empty((n_frames, 13), dtype=torch.float32, device="cuda")
        t = timed(lambda: m.fe_batch_rates_device(d_pcm, off, srs, d_cep), a.reps, torch)
        m.set_kernel_timing(True)
        m.fe_batch_rates_device(d_pcm, off, srs, d_cep)
        ms = m.fe_kernel_timing()
        m.set_kernel_timing(False)
        res["rates"][str(name)] = {"frames": n_frames, "call_ms": round(t * 1e3, 3),
                                   "frames_per_s": round(n_frames / t),
                                   "spectrum_ms": round(ms[0], 3), "noise_ms": round(ms[1], 3),
                                   "cep_ms": round(ms[2], 3)}
        del d_pcm, d_cep
        torch.cuda.empty_cache()

    # ---- audio at 44.1 kHz -> alignment against features -> alignment ----------------------
    srs, pcms = batches[44100]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)
    d_pcm = torch.from_numpy(np.concatenate(pcms)).cuda()
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    words = ("go forward ten meters " * (1 + int(a.seconds * 100) // 280)).split()
    texts = ssw.Texts([words] * a.utts)
    d_cep, fo = m.fe_batch_rates_device(d_pcm, off, 44100)
    d_feats = torch.from_numpy(m.feat_batch(d_cep.cpu().numpy(), utt_off=fo)).cuda()
    box = {}

    def run_text():
        box["t"] = ssw.align_text_batch(m, lex, d_feats, fo, texts)

    def run_audio():
        box["a"] = ssw.align_audio_batch(m, lex, d_pcm, off, texts, samprate=44100)

    t_text = timed(run_text, a.reps, torch)
    t_audio = timed(run_audio, a.reps, torch)
    t_fe = timed(lambda: m.fe_batch_rates_device(d_pcm, off, 44100, d_cep), a.reps, torch)
    same = all(box["t"].status(u) == box["a"].status(u) and
               (box["t"].status(u) != 0 or box["t"].json(u) == box["a"].json(u))
               for u in range(a.utts))
    res["align44100"] = {"workload": f"{a.utts} x {int(fo[-1]) // a.utts} frames at 44.1 kHz, "
                                     f"texts of {len(words)} words",
                         "align_text_batch_ms": round(t_text * 1e3, 2),
                         "align_audio_batch_ms": round(t_audio * 1e3, 2),
                         "fe_batch_rates_ms": round(t_fe * 1e3, 3),
                         "fe_share_of_text": round(t_fe / t_text, 4),
                         "aligned": sum(box["a"].status(u) == 0 for u in range(a.utts)),
                         "same_as_text_path": bool(same)}
    line = json.dumps(res)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
