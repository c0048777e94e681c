#!/usr/bin/env python3
"""Writes tests/golden/vad_results.npz and vad_endpoints.json: the reference library's own voice
activity detector and endpointer, through vad.h and endpointer.h, over the inputs of
tests/vad_common.py.

It compiles tests/harness/vad_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it once per case.  While recording it asserts that the
reference marks between 10 % and 90 % of the frames of every speech fixture as speech: a fixture
whose frames are all one class proves nothing about the model update.

    python tests/golden/make_vad.py           # rewrite the fixtures
    python tests/golden/make_vad.py --check   # rewrite nothing; exit 1 and name every
                                              # fixture whose bytes would change
"""
import io
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import vad_common as V  # noqa: E402


def build_driver(tmp):
    exe = os.path.join(tmp, "vad_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "vad_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def message(stderr):
    """the text of the last ERROR or WARN line of the reference's log, its file and line apart"""
    lines = [ln for ln in stderr.splitlines() if re.match(r"\s*(ERROR|WARN)", ln)]
    assert lines, stderr
    return re.sub(r'^\s*(ERROR|WARN):\s*(".*?", line \d+:\s*)?', "", lines[-1]).strip()


def generate(tmp):
    exe = build_driver(tmp)
    raw = os.path.join(tmp, "pcm.raw")
    out = os.path.join(tmp, "classes.i8")
    arrays, segments, refusals = {}, {}, {}
    for (case, name, mode, rate, fl) in V.VAD_CASES:
        V.stream(name, rate).astype("<i2").tofile(raw)
        r = subprocess.run([exe, "vad", str(mode), str(rate), repr(fl), raw, out], check=True,
                           capture_output=True, text=True)
        frames, size = (int(x) for x in r.stdout.split()[:2])
        dec = np.fromfile(out, dtype=np.int8)
        assert len(dec) == frames and size == V.frame_size(rate, fl), (case, r.stdout)
        if name in V.RECORDINGS:
            assert frames >= 400, (case, frames)
            share = float((dec != 0).mean())
            assert 0.10 <= share <= 0.90, f"{case}: the reference marks {share:.1%} as speech"
        arrays["dec/" + case] = dec
    for c in V.EP_CASES:
        case, _, mode, rate, fl, window, ratio, _ = c
        V.ep_input(c).astype("<i2").tofile(raw)
        r = subprocess.run([exe, "ep", repr(window), repr(ratio), str(mode), str(rate), repr(fl),
                            raw], check=True, capture_output=True, text=True)
        segs = []
        for ln in r.stdout.splitlines():
            first, n, start, end = ln.split()
            segs.append([int(first), int(n), start, end])       # the times as printed
        segments[case] = segs
    for (case, kind, args) in V.REFUSALS:
        r = subprocess.run([exe, "refuse-" + kind] + [repr(a) if isinstance(a, float) else str(a)
                                                      for a in args],
                           check=True, capture_output=True, text=True)
        refusals[case] = message(r.stderr)
    return arrays, {"segments": segments, "refusals": refusals}


def npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def differences(arrays, ep):
    bad = []
    if not os.path.exists(V.RESULTS_NPZ):
        bad.append(V.RESULTS_NPZ)
    else:
        have = np.load(V.RESULTS_NPZ)
        for k, v in arrays.items():
            if (k not in have.files or have[k].dtype != v.dtype or have[k].shape != v.shape
                    or have[k].tobytes() != v.tobytes()):
                bad.append(k)
        bad += [k for k in have.files if k not in arrays]
    if not os.path.exists(V.ENDPOINTS_JSON):
        bad.append(V.ENDPOINTS_JSON)
    else:
        have = json.load(open(V.ENDPOINTS_JSON))
        for part in ("segments", "refusals"):
            a, b = have.get(part, {}), ep[part]
            bad += [f"{part}/{k}" for k in set(a) | set(b) if a.get(k) != b.get(k)]
    return bad


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        arrays, ep = generate(tmp)
    if check:
        bad = differences(arrays, ep)
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(V.RESULTS_NPZ, "wb") as f:
        f.write(npz_bytes(arrays))
    with open(V.ENDPOINTS_JSON, "w") as f:
        json.dump(ep, f, indent=1, sort_keys=True)
        f.write("\n")
    n_seg = sum(len(s) for s in ep["segments"].values())
    print(f"{len(arrays)} decision arrays, {os.path.getsize(V.RESULTS_NPZ)} bytes; "
          f"{len(ep['segments'])} endpointer cases with {n_seg} segments, "
          f"{os.path.getsize(V.ENDPOINTS_JSON)} bytes; {len(ep['refusals'])} refusals")


if __name__ == "__main__":
    main()
