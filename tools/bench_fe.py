"""The MFCC front end on the GPU (ssw_fe_batch, csrc/ssw_k8_fe.inc): what it costs.

    python tools/bench_fe.py [--utts 2048] [--frames 1000] [--reps 5]

Prints one JSON object:
  fe          front-end frames/s for utts x frames of PCM (en-us settings: 20 filters, noise
              removal, DCT, lifter), ms per kernel (spectrum, noise, cepstrum) from HIP events and
              the whole call, device PCM in, device cepstra out
  align       align_audio_batch against align_text_batch at 256 x frames (same audio; the
              features of align_text_batch come from the front end beforehand, untimed)
  noise_page  the serial noise stage on one page-length utterance (~96,000 frames)
  cpu         the CPU restatement of the front end (oracle/ssw_oracle_fe.c) on one utterance of
              `frames` frames, frames/s on one core, for context
Audio: pieces of tests/golden/goforward.raw, scaled and with noise, tiled to length.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def audio(n_utts, n_samples, seed=7):
    go = np.fromfile(os.path.join(ROOT, "tests", "golden", "goforward.raw"), dtype="<i2")
    rng = np.random.default_rng(seed)
    reps = -(-n_samples // len(go))
    base = np.tile(go, reps)[:n_samples].astype(np.float32)
    out = np.empty((n_utts, n_samples), np.int16)
    for u in range(n_utts):
        x = np.roll(base, int(rng.integers(0, len(go)))) * rng.uniform(0.3, 2.0)
        x += rng.normal(0, 50, n_samples).astype(np.float32)
        out[u] = np.clip(np.round(x), -32768, 32767)
    return out.reshape(-1)


def samples_for(frames):
    return 410 + (frames - 2) * 160          # fe_frame_counts() == frames


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
    ap.add_argument("--utts", type=int, default=2048)
    ap.add_argument("--frames", type=int, default=1000)
    ap.add_argument("--align-utts", type=int, default=256)
    ap.add_argument("--page-frames", type=int, default=96000)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch

    import soundswallower_amd as ssw
    from oracle import oracle as O

    mdir = ssw.model_dir("en-us")
    m = ssw.Model(mdir)
    ns = samples_for(a.frames)
    res = {"metric": "front end", "workload": f"{a.utts} x {a.frames} frames of 16 kHz PCM, en-us "
           "feat_params.json (20 filters, remove_noise, dct, lifter 22)"}

    # ---- front end, the big batch ------------------------------------------------------
    pcm = audio(a.utts, ns)
    off = np.arange(a.utts + 1, dtype=np.int64) * ns
    d_pcm = torch.from_numpy(pcm).cuda()
    n_frames = int(ssw.fe_frame_counts(np.diff(off)).sum())
    d_cep = torch.empty((n_frames, 13), dtype=torch.float32, device="cuda")
    t = timed(lambda: m.fe_batch_device(d_pcm, off, d_cep), a.reps, torch)
    m.set_kernel_timing(True)
    m.fe_batch_device(d_pcm, off, d_cep)
    ms = m.fe_kernel_timing()
    m.set_kernel_timing(False)
    res["fe"] = {"frames": n_frames, "call_ms": round(t * 1e3, 3),
                 "frames_per_s": round(n_frames / t), "spectrum_ms": round(ms[0], 3),
                 "noise_ms": round(ms[1], 3), "cep_ms": round(ms[2], 3)}
    del d_pcm, d_cep
    torch.cuda.empty_cache()

    # ---- audio -> alignment against features -> alignment ------------------------------
    k = a.align_utts
    pcm_k = pcm[:k * ns]
    off_k = off[:k + 1]
    d_pcm = torch.from_numpy(pcm_k.copy()).cuda()
    lex = ssw.Lexicon(m, os.path.join(mdir, "dict.txt"), os.path.join(mdir, "noisedict.txt"))
    words = ("go forward ten meters " * (1 + a.frames // 280)).split()
    texts = ssw.Texts([words] * k)
    d_cep, fo = m.fe_batch_device(d_pcm, off_k)
    feats = m.feat_batch(d_cep.cpu().numpy(), utt_off=fo)
    d_feats = torch.from_numpy(feats).cuda()
    box = {}

    def run_text():
        box["t"] = ssw.align_text_batch(m, lex, d_feats, fo, texts)

    def run_audio():
        box["a"] = ssw.align_audio_batch(m, lex, d_pcm, off_k, texts)

    t_text = timed(run_text, a.reps, torch)
    t_audio = timed(run_audio, a.reps, torch)
    t_fe = timed(lambda: m.fe_batch_device(d_pcm, off_k, d_cep), a.reps, torch)
    same = all(box["t"].status(u) == box["a"].status(u) and
               (box["t"].status(u) != 0 or box["t"].json(u) == box["a"].json(u)) for u in range(k))
    res["align"] = {"workload": f"{k} x {a.frames} frames, texts of {len(words)} words",
                    "align_text_batch_ms": round(t_text * 1e3, 2),
                    "align_audio_batch_ms": round(t_audio * 1e3, 2),
                    "fe_batch_ms": round(t_fe * 1e3, 3),
                    "fe_share_of_text": round(t_fe / t_text, 4),
                    "aligned": sum(box["a"].status(u) == 0 for u in range(k)),
                    "same_as_text_path": bool(same)}
    del d_pcm, d_cep, d_feats
    torch.cuda.empty_cache()

    # ---- one page-length utterance: the serial noise stage --------------------------------
    nsp = samples_for(a.page_frames)
    d_page = torch.from_numpy(audio(1, nsp, seed=9)).cuda()
    off_p = np.array([0, nsp], np.int64)
    d_cep = torch.empty((a.page_frames, 13), dtype=torch.float32, device="cuda")
    t_page = timed(lambda: m.fe_batch_device(d_page, off_p, d_cep), a.reps, torch)
    m.set_kernel_timing(True)
    m.fe_batch_device(d_page, off_p, d_cep)
    ms = m.fe_kernel_timing()
    m.set_kernel_timing(False)
    res["noise_page"] = {"frames": a.page_frames, "call_ms": round(t_page * 1e3, 3),
                         "spectrum_ms": round(ms[0], 3), "noise_ms": round(ms[1], 3),
                         "cep_ms": round(ms[2], 3),
                         "noise_us_per_frame": round(ms[1] * 1e3 / a.page_frames, 4)}

    # ---- the CPU restatement, one core ----------------------------------------------------
    one = pcm[:ns]
    O.fe_mfcc(one[:4000], nfilt=20, lowerf=130, upperf=3700, lifter=22, remove_noise=True,
              transform="dct")
    t0 = time.perf_counter()
    cep = O.fe_mfcc(one, nfilt=20, lowerf=130, upperf=3700, lifter=22, remove_noise=True,
                    transform="dct")
    t_cpu = time.perf_counter() - t0
    res["cpu"] = {"frames": len(cep), "ms": round(t_cpu * 1e3, 2),
                  "frames_per_s_one_core": round(len(cep) / t_cpu)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
