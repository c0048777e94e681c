"""Dynamic features of every configuration: the recorded reference cases, a plain restatement,
and the test model C1-lda.

restate() restates feat_s2mfc2feat_block_utt (src/feat.c:977-1008) in numpy float32, one
operation a rounding, with explicit sequential loops where the reference has them:
  cmn             src/cmn.c:159-224      the mean's sum frame after frame (frames with c0 < 0
                                         skipped), the variance over all frames, the scale
                                         (float)sqrt((double)n / var)
  cmn_live,       src/cmn_live.c:60-134  the prior subtracted in frames with c0 >= 0, the sum
  cmn_live_update                        frame after frame, the shift (nframe > 800, >= inside)
                                         and the update at the utterance's end (> 800)
  compute_feat    src/feat.c:437-712     every type as its function writes it
  the LDA         src/lda.c:124-144      tmp[j] += x[k] * lda[j][k], k ascending
  the gather      src/feat.c:346-366
resolve() restates feat_init_s3file's chain of comparisons (src/feat.c:749-884).

The cases (CASES) were recorded from the reference library by tests/golden/make_feat_types.py
through tests/harness/feat_types_driver.c; cases() loads them.
"""
from __future__ import annotations

import json
import os
import re
import struct

import numpy as np

from tests import sc_common as S

ROOT = S.ROOT
GOLD = S.GOLD
DIR = os.path.join(GOLD, "feat_types")
CASES_JSON = os.path.join(DIR, "cases.json")
MFCC = os.path.join(GOLD, "goforward_mfcc.npy")
LDA_FILE = os.path.join(DIR, "feature_transform")      # the reference's tests/data file: 36 x 39
LENS = (1, 2, 3, 4, 5, 9, 40)
CMN_WIN, CMN_WIN_HWM = 500, 800
F32 = np.float32
INIT13 = "41.0,-5.25,-0.12,5.43,2.78,-1.84,-0.84,-1.97,-0.83,-2.72,-2.97,-1.5,0.2"

_BATCH = {"cmn": "batch"}


def _c(file, settings, lens=LENS, mode="fresh", inp="mfcc"):
    return {"file": file, "settings": settings, "lens": list(lens), "mode": mode, "input": inp}


# name -> the npz file it is kept in, the settings (over the reference's defaults: 1s_c_d_dd,
# ceplen 13, cmn live, cmninit 40,3,-1), the utterances, the mode and the input
CASES = {
    # every feature type, at cmn = batch
    "s2_4x": _c("types", dict(_BATCH, feat="s2_4x")),
    "s3_1x39": _c("types", dict(_BATCH, feat="s3_1x39")),
    "1s_12c_12d_3p_12dd": _c("types", dict(_BATCH, feat="1s_12c_12d_3p_12dd")),
    "1s_c_d_dd": _c("types", dict(_BATCH, feat="1s_c_d_dd")),
    "1s_c_d_ld_dd": _c("types", dict(_BATCH, feat="1s_c_d_ld_dd")),
    "cep_dcep": _c("types", dict(_BATCH, feat="cep_dcep")),
    "1s_c_d": _c("types", dict(_BATCH, feat="1s_c_d")),
    "cep": _c("types", dict(_BATCH, feat="cep")),
    "1s_c": _c("types", dict(_BATCH, feat="1s_c")),
    "1s_3c": _c("types", dict(_BATCH, feat="1s_3c")),
    "1s_4c": _c("types", dict(_BATCH, feat="1s_4c")),
    "generic_13": _c("types", dict(_BATCH, feat="13")),
    "generic_13_2": _c("types", dict(_BATCH, feat="13:2")),
    "generic_4_9_1": _c("types", dict(_BATCH, feat="4,9:1")),
    # 1s_c_d_dd under every CMN mode
    "cmn_none": _c("cmn", {"cmn": "none"}),
    "cmn_batch_varnorm": _c("cmn", dict(_BATCH, varnorm="yes")),
    "cmn_live": _c("cmn", {}),
    "cmn_live_init13": _c("cmn", {"cmninit": INIT13}),
    "cmn_prior_alias": _c("cmn", {"cmn": "prior", "cmninit": "12.5"}),
    # c0 < 0 in some frames: cmn and cmn_live skip them
    "negc0_batch": _c("cmn", dict(_BATCH), inp="negc0"),
    "negc0_varnorm": _c("cmn", dict(_BATCH, varnorm="yes"), inp="negc0"),
    "negc0_live": _c("cmn", {}, inp="negc0"),
    # LDA and svspec
    "lda_0": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=0)),
    "lda_12": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=12)),
    "lda_29": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=29)),
    "lda_99": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=99)),
    "sv_permute": _c("lda", dict(_BATCH, svspec="24,0-11/25,12-23/26-38")),
    "lda_29_sv": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=29, svspec="28,0-9/10-20,27")),
    "lda_12_sv_beyond": _c("lda", dict(_BATCH, lda=LDA_FILE, ldadim=12, svspec="0-5/30,11")),
    "lda_live": _c("lda", dict(lda=LDA_FILE, ldadim=29)),
    # one decoder's utterances in order under cmn = live
    "chain": _c("chain", {}, lens=(200, 150, 100), mode="chain", inp="double"),
    "chain_empty": _c("chain", {"cmninit": INIT13}, lens=(120, 0, 250, 40), mode="chain", inp="double"),
}


def mfcc():
    return np.load(MFCC).astype(F32)


def case_input(case):
    """the cepstra a case's utterances are cut from, back to back"""
    n = sum(case["lens"])
    m = mfcc()
    if case["input"] == "double":
        return np.ascontiguousarray(np.concatenate([m, m])[:n])
    cep = np.ascontiguousarray(m[:n])
    if case["input"] == "negc0":
        cep[2::5, 0] = -np.abs(cep[2::5, 0]) - F32(1)
    return cep


def offsets(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)


def cases():
    """the recorded cases: name -> dict(settings, lens, mode, input, dims, out float32
    [frames][width], state float32 [n_utts][2 ceplen] and nframe int32 [n_utts] after every
    utterance, when the configuration has a CMN)"""
    with open(CASES_JSON, encoding="utf-8") as fh:
        meta = json.load(fh)["cases"]
    files = {}
    got = {}
    for name, rec in meta.items():
        z = files.setdefault(rec["file"], np.load(os.path.join(DIR, rec["file"] + ".npz")))
        rec = dict(rec)
        rec["settings"] = localize(rec["settings"])
        rec["out"] = z[name].reshape(-1, rec["dims"]["width"])
        if name + ".state" in z.files:
            rec["state"] = z[name + ".state"]
            rec["nframe"] = z[name + ".nframe"]
        got[name] = rec
    return got


def e2e():
    with open(CASES_JSON, encoding="utf-8") as fh:
        return json.load(fh)["e2e"]


def portable(settings):
    """settings as they are recorded: the LDA file by its name"""
    return {k: (os.path.basename(v) if k == "lda" else v) for k, v in settings.items()}


def localize(settings):
    return {k: (os.path.join(DIR, v) if k == "lda" else v) for k, v in settings.items()}


# ------------------------------------------------------------------------------------------
# the configuration, restated
# ------------------------------------------------------------------------------------------
DEFAULTS = {"feat": "1s_c_d_dd", "ceplen": 13, "cmn": "live", "cmninit": "40,3,-1", "varnorm": "no",
            "lda": None, "ldadim": 0, "svspec": None}
CMN = {"none": "none", "batch": "batch", "current": "batch", "live": "live", "prior": "live"}


def read_lda(path):
    """matrix 0 of an s3 transform file, float32 [rows][cols]"""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"endhdr\n") + len(b"endhdr\n")
    assert struct.unpack_from("<I", blob, end)[0] == 0x11223344
    n, rows, cols, total = struct.unpack_from("<4i", blob, end + 4)
    assert total == n * rows * cols
    return np.frombuffer(blob, "<f4", rows * cols, end + 20).reshape(rows, cols).astype(F32)


def write_lda(path, mat):
    mat = np.ascontiguousarray(mat, "<f4")
    S.write_s3(path, struct.pack("<4i", 1, mat.shape[0], mat.shape[1], mat.size) + mat.tobytes())


def parse_svspec(spec):
    return [[d for part in sv.split(",") for d in
             (lambda a, b=None: range(int(a), int(b if b is not None else a) + 1))(*part.split("-"))]
            for sv in spec.split("/")]


def resolve(settings):
    """dict(kind, ceplen, window, streams (lengths), raw, cmn, varnorm, lda (used rows, float32
    [rows][raw]) or None, sv (list of lists) or None, width, prior (mean, sum, nframe))"""
    s = dict(DEFAULTS, **settings)
    t, c = s["feat"], int(s["ceplen"]) or 13
    if t == "s2_4x":
        kind, streams, win = "s2_4x", [12, 24, 3, 12], 4
    elif t in ("s3_1x39", "1s_12c_12d_3p_12dd"):
        kind, streams, win = "s3_1x39", [39], 3
    elif t.startswith("1s_c_d_dd"):
        kind, streams, win = "c_d_dd", [3 * c], 3
    elif t.startswith("1s_c_d_ld_dd"):
        kind, streams, win = "c_d_ld_dd", [4 * c], 4
    elif t.startswith("cep_dcep") or t.startswith("1s_c_d"):
        kind, streams, win = "c_d", [2 * c], 2
    elif t.startswith("cep") or t.startswith("1s_c"):
        kind, streams, win = "c", [c], 0
    elif t.startswith("1s_3c") or t.startswith("1s_4c"):
        win = 3 if t.startswith("1s_3c") else 4
        kind, streams = "copy", [c * (2 * win + 1)]
    else:
        m = re.fullmatch(r"(\d+(?:,\d+)*)(?::(\d+))?", t)
        assert m, "the restatement takes well-formed generic types only"
        win = int(m.group(2) or 0)
        base = [int(x) for x in m.group(1).split(",")]
        assert sum(base) == c
        kind, streams = "copy", [b * (2 * win + 1) for b in base]
    r = dict(kind=kind, ceplen=c, window=win, streams=streams, raw=sum(streams), cmn=CMN[s["cmn"]],
             varnorm=str(s["varnorm"]).lower() in ("yes", "true", "1"), lda=None, sv=None)
    r["width"] = r["raw"]
    if s["lda"]:
        mat = read_lda(s["lda"])
        dim = int(s["ldadim"])
        rows = mat.shape[0] if dim <= 0 or dim > mat.shape[0] else dim
        assert mat.shape[1] == streams[0] and len(streams) == 1
        r["lda"] = mat[:rows]
        r["width"] = rows
    if s["svspec"]:
        r["sv"] = parse_svspec(s["svspec"])
        r["width"] = sum(len(v) for v in r["sv"])
    mean = np.zeros(c, F32)
    total = np.zeros(c, F32)
    nframe = 0
    if r["cmn"] != "none" and s["cmninit"]:       # cmn_set_repr, src/cmn.c:112-140
        vals = s["cmninit"].split(",")
        for i, v in enumerate(vals[:c]):
            if v == "" and i == len(vals) - 1:
                break
            mean[i] = F32(float(v))
        total = mean * F32(CMN_WIN)
        nframe = CMN_WIN
    r["prior"] = (mean, total, nframe)
    return r


# ------------------------------------------------------------------------------------------
# the computation, restated
# ------------------------------------------------------------------------------------------
def _live_renew(mean, total, nframe, inclusive):
    """cmn_live_shiftwin (inclusive) / cmn_live_update's body, src/cmn_live.c:60-104"""
    with np.errstate(all="ignore"):
        sf = F32(1.0) / F32(nframe)
        mean = total / F32(nframe)
        if (nframe >= CMN_WIN_HWM) if inclusive else (nframe > CMN_WIN_HWM):
            sf = F32(CMN_WIN) * sf
            total = total * sf
            nframe = CMN_WIN
    return mean.astype(F32), total.astype(F32), nframe


def _normalise(x, r, state):
    """feat_cmn over one whole utterance (in place on a copy); returns (x, state after)"""
    x = x.copy()
    n, c = x.shape
    if r["cmn"] == "none" or n == 0 and r["cmn"] == "batch":
        return x, state
    mean, total, nframe = state
    with np.errstate(all="ignore"):
        if r["cmn"] == "batch":
            total = np.zeros(c, F32)
            nframe = 0
            for f in range(n):
                if x[f, 0] < 0:
                    continue
                total = total + x[f]
                nframe += 1
            mean = total / F32(nframe)
            if not r["varnorm"]:
                x = x - mean
            else:
                var = np.zeros(c, F32)
                for f in range(n):
                    t = x[f] - mean
                    var = var + t * t
                scale = np.sqrt(np.float64(n) / var.astype(np.float64)).astype(F32)
                x = (x - mean) * scale
            return x.astype(F32), (mean, total, nframe)
        if n > 0:
            for f in range(n):
                if x[f, 0] < 0:
                    continue
                total = total + x[f]
                x[f] = x[f] - mean
                nframe += 1
            if nframe > CMN_WIN_HWM:
                mean, total, nframe = _live_renew(mean, total, nframe, True)
        if nframe > 0:
            mean, total, nframe = _live_renew(mean, total, nframe, False)
    return x, (mean, total, nframe)


def _raw(x, r):
    """compute_feat for every frame of one normalised utterance: float32 [n][raw]"""
    n, c = x.shape
    w = r["window"]
    pad = np.concatenate([np.repeat(x[:1], w, 0), x, np.repeat(x[-1:], w, 0)])
    at = lambda o, lo=0, hi=None: pad[w + o:w + o + n, lo:hi]
    d = lambda o, lo=0, hi=None: at(o, lo, hi) - at(-o, lo, hi)
    dd = lambda lo=0, hi=None: (at(3, lo, hi) - at(-1, lo, hi)) - (at(1, lo, hi) - at(-3, lo, hi))
    k = r["kind"]
    if k == "s2_4x":
        parts = [at(0, 1), d(2, 1), d(4, 1), at(0, 0, 1), d(2, 0, 1), dd(0, 1), dd(1)]
    elif k == "s3_1x39":
        parts = [at(0, 1), d(2, 1), at(0, 0, 1), d(2, 0, 1), dd(0, 1), dd(1)]
    elif k == "c_d_dd":
        parts = [at(0), d(2), dd()]
    elif k == "c_d_ld_dd":
        parts = [at(0), d(2), d(4), dd()]
    elif k == "c_d":
        parts = [at(0), d(2)]
    elif k == "c":
        parts = [at(0)]
    else:
        parts, lo = [], 0
        for sl in r["streams"]:
            sl //= 2 * w + 1
            parts += [at(o, lo, lo + sl) for o in range(-w, w + 1)]
            lo += sl
    return np.concatenate(parts, axis=1).astype(F32)


def _project(raw, r):
    y = raw
    if r["lda"] is not None:
        lda = r["lda"]
        y = np.zeros((len(raw), len(lda)), F32)
        for k in range(raw.shape[1]):
            y = y + raw[:, k:k + 1] * lda[None, :, k]
    if r["sv"] is not None:
        full = np.zeros((len(raw), raw.shape[1]), F32)   # the row behind an LDA: zeros past its rows
        full[:, :y.shape[1]] = y
        y = full[:, [d for sv in r["sv"] for d in sv]]
    return np.ascontiguousarray(y, F32)


def restate(cep, utt_off, settings, state=None):
    """(features float32 [n][width], states after every utterance as a list of (mean, sum,
    nframe)).  state None: every utterance is a fresh decoder's first; else (mean, sum, nframe),
    and the utterances are one decoder's in order (cmn = live)."""
    r = resolve(settings)
    cep = np.asarray(cep, F32)
    out, states = [], []
    cur = state
    for u in range(len(utt_off) - 1):
        x = cep[utt_off[u]:utt_off[u + 1]]
        st = cur if state is not None and r["cmn"] == "live" else r["prior"]
        xn, after = _normalise(x, r, (st[0].copy(), st[1].copy(), st[2]))
        states.append(after)
        cur = after
        if len(x):
            out.append(_project(_raw(xn, r), r))
    width = r["width"]
    return (np.concatenate(out) if out else np.zeros((0, width), F32)), states


def state_tuple(s):
    """an SswCmnState -> (mean, sum, nframe) over 64 dimensions"""
    return np.array(s.mean[:], F32), np.array(s.sum[:], F32), int(s.nframe)


# ------------------------------------------------------------------------------------------
# the tile table, restated
# ------------------------------------------------------------------------------------------
def tiles(utt_off, tf):
    return [(u, f) for u in range(len(utt_off) - 1) for f in range(utt_off[u], utt_off[u + 1], tf)]


# ------------------------------------------------------------------------------------------
# model C1-lda: cont_common's C1 behind a transform whose products and sums are exact
# ------------------------------------------------------------------------------------------
LDA_ROWS = 32
LDA_SEED = 20261020


def c1_lda_matrix(drop=None):
    """float32 [32][39]: row j holds one entry, +-2^e (e in -1, 0, 1), at column perm[j]; the 7
    columns left out are `drop` (default: the last delta-delta dimensions)"""
    rng = np.random.default_rng(LDA_SEED)
    drop = list(range(32, 39)) if drop is None else list(drop)
    keep = [k for k in range(39) if k not in drop]
    perm = rng.permutation(keep)
    val = (rng.choice([-1.0, 1.0], LDA_ROWS) * np.exp2(rng.integers(-1, 2, LDA_ROWS))).astype(F32)
    mat = np.zeros((LDA_ROWS, 39), F32)
    mat[np.arange(LDA_ROWS), perm] = val
    return mat, perm, val


def model_c1_lda_dir(d, matrix=None, permute=True):
    """C1 with a feature_transform beside its means: means permuted and scaled to match,
    variances scaled by the square, ldadim 32.  matrix: another transform to write (the refusal:
    the real 36-row one, with the 39-dimensional means kept)."""
    from tests import cont_common as CC
    CC.model_c1_dir(d)
    with open(os.path.join(d, "feat_params.json"), encoding="utf-8") as fh:
        fp = json.load(fh)
    mat, perm, val = c1_lda_matrix()
    if permute:
        _, _, (mean,) = S.read_gauss(os.path.join(d, "means"))
        _, _, (var,) = S.read_gauss(os.path.join(d, "variances"))
        S.write_gauss(os.path.join(d, "means"), [(mean[:, :, perm] * val).astype(F32)])
        S.write_gauss(os.path.join(d, "variances"), [(var[:, :, perm] * (val * val)).astype(F32)])
        fp["ldadim"] = LDA_ROWS
    with open(os.path.join(d, "feat_params.json"), "w", encoding="utf-8") as fh:
        json.dump(fp, fh, indent=0)
        fh.write("\n")
    write_lda(os.path.join(d, "feature_transform"), mat if matrix is None else matrix)
    return d
