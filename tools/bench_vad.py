"""Voice activity detection and endpointing of a batch of streams (csrc/ssw_k13_vad.inc) beside the
reference's own vad_classify loop on one host core.

    python tools/bench_vad.py [--streams 2048] [--seconds 10] [--reps 7] [--out profiles/vad_batch.json]

The batch is `streams` streams of `seconds` s at 16 kHz, 30 ms frames, mode 0, made by tiling the
committed recordings (each stream starts at its own offset into them).  Recorded, each the median,
minimum and maximum of `reps` calls after a warm-up, samples on the device:
  vad_batch_ms       ssw_vad_batch between two device events (the offsets' upload, the kernel, the
                     final synchronise), at the launch's own streams per workgroup and at every
                     other value ssw_vad_set_streams_per_workgroup takes, alternating
  one_stream_ms      the same call on the first stream alone: one lane of one wave
  endpoint_batch_ms  ssw_endpoint_batch by the host clock: the same, the decisions brought to the
                     host and the endpointer's replay per stream
  host_path_ms       ssw_vad_batch_host over `ref-streams` of the streams on one core
  reference          tests/harness/vad_driver.c in its `time` mode over the same `ref-streams`
                     streams, linked against oracle/_ref/ on this machine (null when build() made
                     no reference library): seconds of the best of 5 passes, per stream and scaled
                     to the batch.  The parent of this feature has no path to compare with, so the
                     reference is the yardstick.
The decisions of the timed call are checked against the host path's on the `ref-streams` streams
before anything is reported.  Prints the JSON and writes it to --out."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(streams, samples):
    gold = os.path.join(ROOT, "tests", "golden")
    recs = [np.fromfile(os.path.join(gold, n + ".raw"), dtype="<i2") for n in ("goforward", "goforward_fr")]
    out = np.empty((streams, samples), np.int16)
    for u in range(streams):
        r = recs[u % 2]
        start = (u * 997) % len(r)
        out[u] = np.tile(r, samples // len(r) + 2)[start:start + samples]
    return out


def stats(ts):
    return {"median": round(float(np.median(ts)), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


def reference_seconds(pcm, reps=5):
    """the reference's vad_classify loop over pcm's streams, one after the other, on one core"""
    from oracle import reference
    if not reference.available():
        return None
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "vad_driver")
        subprocess.run(["gcc", "-O2", "-std=gnu99", "-I" + reference.INCLUDE, "-I" + reference.BUILD,
                        os.path.join(ROOT, "tests", "harness", "vad_driver.c"), reference.LIBRARY,
                        "-lm", "-o", exe], check=True)
        raw = os.path.join(tmp, "pcm.raw")
        total = 0.0
        for u in range(len(pcm)):           # a fresh vad_t per stream, as a caller would make it
            pcm[u].astype("<i2").tofile(raw)
            r = subprocess.run([exe, "time", "0", "16000", "0.03", raw, str(reps)], check=True,
                               capture_output=True, text=True)
            total += float(r.stdout.split()[0])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=2048)
    ap.add_argument("--seconds", type=float, default=10.0)
    ap.add_argument("--ref-streams", type=int, default=32)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vad_batch.json"))
    a = ap.parse_args()
    import torch

    import soundswallower_amd as ssw

    if not torch.cuda.is_available():
        sys.exit("bench_vad: no GPU; nothing is measured without one")
    samples = int(a.seconds * 16000)
    pcm = batch(a.streams, samples)
    off = np.arange(a.streams + 1, dtype=np.int64) * samples
    d_pcm = torch.from_numpy(pcm.reshape(-1)).cuda()
    vad = ssw.Vad(0, 16000, 0.03)
    L = vad._L
    n_frames = a.streams * (samples // vad.frame_size)
    d_dec = torch.empty(n_frames, dtype=torch.int8, device="cuda")
    frame_off = np.zeros(a.streams + 1, np.int32)

    def run():
        rv = L.ssw_vad_batch(vad._h, d_pcm.data_ptr(), off.ctypes.data, a.streams, d_dec.data_ptr(),
                             frame_off.ctypes.data, None, None)
        assert rv == 0, ssw.api._lib.last_error()

    # parity first: the device's decisions on the first streams are the host path's
    k = min(a.ref_streams, a.streams)
    run()
    t0 = time.perf_counter()
    want, fo = vad.classify_batch_host(pcm[:k].reshape(-1), off[:k + 1])
    host_ms = (time.perf_counter() - t0) * 1e3
    got = d_dec[:fo[-1]].cpu().numpy()
    assert np.array_equal(got, want), "device decisions differ from the host path"

    speech_share = round(float((d_dec != 0).float().mean()), 4)   # of the whole batch's frames
    settings = [0, 8, 16, 32, 64]             # 0: the launch's own choice
    times = {s: [] for s in settings}
    for s in settings:                        # warm-up of every shape
        vad.set_streams_per_workgroup(s)
        run()
    for _ in range(a.reps):                   # alternating
        for s in settings:
            vad.set_streams_per_workgroup(s)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            torch.cuda.synchronize()
            times[s].append(e0.elapsed_time(e1))
    vad.set_streams_per_workgroup(0)
    one = []                                  # one stream: one lane of one wave
    for i in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rv = L.ssw_vad_batch(vad._h, d_pcm.data_ptr(), off.ctypes.data, 1, d_dec.data_ptr(),
                             frame_off.ctypes.data, None, None)
        e1.record()
        torch.cuda.synchronize()
        assert rv == 0
        if i:
            one.append(e0.elapsed_time(e1))
    ep = []
    n_segs = 0
    for i in range(a.reps + 1):
        t0 = time.perf_counter()
        h = L.ssw_endpoint_batch(vad._h, 0.3, 0.9, d_pcm.data_ptr(), off.ctypes.data, a.streams, None)
        if i:
            ep.append((time.perf_counter() - t0) * 1e3)
        assert h, ssw.api._lib.last_error()
        n_segs = sum(L.ssw_endpoints_count(h, u) for u in range(a.streams))
        L.ssw_endpoints_free(h)
    ref_s = reference_seconds(pcm[:k])
    audio_s = a.streams * a.seconds
    med = float(np.median(times[0]))
    res = {"metric": "voice activity detection of a batch of streams",
           "workload": f"{a.streams} streams x {a.seconds:g} s of 16 kHz PCM tiled from the committed "
                       "recordings, 30 ms frames, mode 0",
           "frames": n_frames, "speech_share": speech_share,
           "reps": a.reps,
           "vad_batch_ms": stats(times[0]),
           "vad_batch_ms_by_streams_per_workgroup": {str(s): stats(times[s]) for s in settings if s},
           "one_stream_ms": stats(one),
           "audio_seconds_per_second": round(audio_s / (med * 1e-3)),
           "endpoint_batch_ms": stats(ep), "segments": n_segs,
           "host_path_ms": {"streams": k, "ms": round(host_ms, 3),
                            "scaled_to_batch_ms": round(host_ms * a.streams / k, 1)},
           "reference": None if ref_s is None else {
               "what": "vad_classify loop of the reference library, one host core, best of 5",
               "streams": k, "ms_per_stream": round(ref_s * 1e3 / k, 3),
               "scaled_to_batch_ms": round(ref_s * 1e3 * a.streams / k, 1),
               "batch_speedup": round(ref_s * 1e3 * a.streams / k / med, 1)}}
    print(json.dumps(res))
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
