#!/usr/bin/env python3
"""Writes tests/golden/fe_any_mfcc.npz and fe_any_align.json: the reference library's own front
end under the settings that only ssw_fe_batch_any takes (remove_dc, any alpha, htk, any ncep,
logspec, smoothspec, doublebw, unit_area, round_filters, frequency warping), and its aligner on
a model directory that declares some of them.

It compiles tests/harness/fe_any_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it once per fixture of tests/fe_any_common.py -- a
process each, because the reference keeps warp parameters in process-wide statics.

    python tests/golden/make_fe_any.py           # rewrite the fixtures
    python tests/golden/make_fe_any.py --check   # rewrite nothing; exit 1 and name every
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
from tests import fe_any_common as A  # noqa: E402
from tests import fe_rates_common as R  # noqa: E402


def build_driver(tmp):
    exe = os.path.join(tmp, "fe_any_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "fe_any_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def generate(tmp):
    exe = build_driver(tmp)
    arrays = {}
    raw = os.path.join(tmp, "pcm.raw")
    out = os.path.join(tmp, "rows.f32")
    for fx in A.FIXTURES:
        name, rate, cfg, _, kind = fx
        A.fixture_pcm(fx).tofile(raw)
        r = subprocess.run([exe, "fe", A.reference_json(cfg, rate), A.KINDS[kind][0], raw, out],
                           check=True, capture_output=True, text=True)
        frames, width = (int(x) for x in r.stdout.split())
        arrays["cep/" + name] = np.fromfile(out, dtype=np.float32).reshape(frames, width)
    R.goforward().astype("<i2").tofile(raw)
    hmm = A.align_model_dir(os.path.join(tmp, "en-us-changed"))
    align = {}
    for comp in A.CONFIGS:
        r = subprocess.run([exe, "align", hmm, comp, raw], check=True, capture_output=True,
                           text=True)
        align[comp] = r.stdout                      # as decoder_result_json returns it
    return arrays, align


def npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def differences(arrays, align):
    """the fixtures whose committed bytes differ from what the reference makes now"""
    bad = []
    if not os.path.exists(A.MFCC_NPZ):
        bad.append(A.MFCC_NPZ)
    else:
        have = np.load(A.MFCC_NPZ)
        for k, v in arrays.items():
            if (k not in have.files or have[k].dtype != v.dtype or have[k].shape != v.shape
                    or have[k].tobytes() != v.tobytes()):
                bad.append(k)
        bad += [k for k in have.files if k not in arrays]
    if not os.path.exists(A.ALIGN_JSON):
        bad.append(A.ALIGN_JSON)
    else:
        have = json.load(open(A.ALIGN_JSON))
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
    with open(A.MFCC_NPZ, "wb") as f:
        f.write(npz_bytes(arrays))
    with open(A.ALIGN_JSON, "w") as f:
        json.dump(align, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(arrays)} arrays, {os.path.getsize(A.MFCC_NPZ)} bytes; {len(align)} alignments")


if __name__ == "__main__":
    main()
