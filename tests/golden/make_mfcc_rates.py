#!/usr/bin/env python3
"""Writes tests/golden/fe_rates_mfcc.npz and fe_rates_align.json: the reference library's own
front end and aligner at sample rates other than 16 kHz, the truth that the front end at any
rate (ssw_fe_batch_ex) is tested against.

It compiles tests/harness/fe_rates_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it on goforward resampled as tests/fe_rates_common.py
resamples it.  fe_rates_mfcc.npz holds, per fixture of fe_rates_common.FIXTURES, the float32
cepstra as "cep/<name>", and per rate the frame counts of n = 1 .. size + 3 shift samples as
"counts/<rate>"; fe_rates_align.json holds decoder_result_json at align_level 1 for goforward
aligned to "go forward ten meters" with the en-us model, per rate and compallsen.

    python tests/golden/make_mfcc_rates.py           # rewrite the fixtures
    python tests/golden/make_mfcc_rates.py --check   # rewrite nothing; exit 1 and name every
                                                     # fixture whose bytes would change
"""
import io
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import fe_rates_common as R  # noqa: E402

MODEL_EN = os.path.join(ROOT, "soundswallower_amd", "model", "en-us")


def build_driver(tmp):
    exe = os.path.join(tmp, "fe_rates_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "fe_rates_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def generate(tmp):
    exe = build_driver(tmp)
    arrays = {}
    raw = os.path.join(tmp, "pcm.raw")
    out = os.path.join(tmp, "cep.f32")
    for name, rate, cfg, spec in R.FIXTURES:
        R.fixture_pcm(spec, rate).astype("<i2").tofile(raw)
        r = subprocess.run([exe, "fe", R.reference_json(cfg, rate), raw, out], check=True,
                           capture_output=True, text=True)
        cep = np.fromfile(out, dtype=np.float32).reshape(-1, 13)
        assert len(cep) == int(r.stdout), name
        arrays["cep/" + name] = cep
    for rate in R.RATES:
        R.resample(R.goforward(), rate).astype("<i2").tofile(raw)
        r = subprocess.run([exe, "count", R.reference_json({}, rate), raw, str(R.count_limit(rate))],
                           check=True, capture_output=True, text=True)
        arrays[f"counts/{rate}"] = np.array([int(x) for x in r.stdout.split()], np.int32)
    align = {}
    for rate in R.ALIGN_RATES:
        R.resample(R.goforward(), rate).astype("<i2").tofile(raw)
        for comp in ("yes", "no"):
            r = subprocess.run([exe, "align", MODEL_EN, str(rate), comp, raw], check=True,
                               capture_output=True, text=True)
            align[f"{rate}/{comp}"] = r.stdout          # as decoder_result_json returns it
    return arrays, align


def npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def differences(arrays, align):
    """the fixtures whose committed bytes differ from what the reference makes now"""
    bad = []
    if not os.path.exists(R.MFCC_NPZ):
        bad.append(R.MFCC_NPZ)
    else:
        have = np.load(R.MFCC_NPZ)
        for k, v in arrays.items():
            if k not in have.files or have[k].dtype != v.dtype or have[k].tobytes() != v.tobytes():
                bad.append(k)
        bad += [k for k in have.files if k not in arrays]
    if not os.path.exists(R.ALIGN_JSON):
        bad.append(R.ALIGN_JSON)
    else:
        have = json.load(open(R.ALIGN_JSON))
        bad += [k for k in set(align) | set(have) if have.get(k) != align.get(k)]
    return bad


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        arrays, align = generate(tmp)
    if check:
        bad = differences(arrays, align)
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(R.MFCC_NPZ, "wb") as f:
        f.write(npz_bytes(arrays))
    with open(R.ALIGN_JSON, "w") as f:
        json.dump(align, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(arrays)} arrays, {os.path.getsize(R.MFCC_NPZ)} bytes; {len(align)} alignments")


if __name__ == "__main__":
    main()
