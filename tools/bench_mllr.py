#!/usr/bin/env python3
"""Times ssw_model_apply_mllr: en-us (PTM, 42 x 3 x 128 densities), C3 (continuous, 5126 senones
x 3 x 8) and a C1 of 32 densities (continuous, 5126 x 1 x 32 of 39 dimensions), on a
SSW_DEVICE_NONE model and on a device model.  Each apply is split into the host transform +
table rebuild and the upload (synchronise + copies), as the library times them
(ssw_model_mllr_timing).  Writes profiles/mllr_apply.json.

    python tools/bench_mllr.py [--reps 9] [--no-gpu] [--out profiles/mllr_apply.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import soundswallower_amd as ssw  # noqa: E402
from tests import cont_common as CC  # noqa: E402
from tests import mllr_common as M  # noqa: E402


def time_model(kwargs, layout, device, reps):
    m = M.load(kwargs, device)
    ts = [ssw.Mllr.read(M.transform_path(n, layout)) for n in ("mild", "var")]
    host, up, wall = [], [], []
    for r in range(reps + 1):  # (the first apply is the warm-up)
        t0 = time.perf_counter()
        m.apply_mllr(ts[r & 1])
        w = (time.perf_counter() - t0) * 1e3
        h, u = m.mllr_timing()
        if r:
            host.append(h), up.append(u), wall.append(w)
    shape = {"n_cb": m.n_cb, "n_feat": m.n_feat, "n_density": m.n_density,
             "veclen_total": m.veclen_total}
    m.close()
    med = statistics.median
    return shape, {"host_ms": round(med(host), 3), "upload_ms": round(med(up), 3),
                   "wall_ms": round(med(wall), 3), "host_ms_min": round(min(host), 3),
                   "host_ms_max": round(max(host), 3), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--no-gpu", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mllr_apply.json"))
    a = ap.parse_args()
    out = {"what": "ssw_model_apply_mllr: median ms of --reps applies alternating two transforms; "
                   "host = transform + rebuild of every derived table, upload = device "
                   "synchronise + copies into the load's allocations", "models": {}}
    with tempfile.TemporaryDirectory() as tmp:
        cases = {"en-us": ({"path": M.S.EN_US}, "3x13"),
                 "C3": (CC.model_paths(CC.model_c3_dir(os.path.join(tmp, "C3"))), "3x13"),
                 "C1_32": (CC.model_paths(CC.model_c1_dir(os.path.join(tmp, "C1_32"), 32, 32)),
                           "1x39")}
        for name, (kw, layout) in cases.items():
            shape, none = time_model(kw, layout, ssw.SSW_DEVICE_NONE, a.reps)
            rec = dict(shape, host_only=none)
            if not a.no_gpu:
                rec["device"] = time_model(kw, layout, -1, a.reps)[1]
            out["models"][name] = rec
            print(name, json.dumps(rec))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w", encoding="utf-8") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
