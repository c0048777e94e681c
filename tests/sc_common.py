"""Semi-continuous (single-codebook) test models and a plain restatement of the s2_semi scorer.

The writers make s3 Gaussian files and an 8-bit sendump; the builders make the models of the
s2_semi tests as pure functions of a seed through soundswallower_amd.synth.lcg_uniform; score()
restates src/s2_semi_mgau.c frame by frame, density by density, in numpy float32 / Python ints:

  model A       en-us with means / variances cut down to codebook 41 (tests/golden/sc/en-us-cb41)
  model A-ties  model A with density 9 copied over 10, 40, 41, 42, 100 and density 3 over 2 in
                every stream: equal truncated scores at the list's boundary (a codebook of 128
                densities has no density 200: 100 stands for it, a tie in the second 64)
  model B       one codebook of 4 streams (12, 24, 3, 12 dimensions, s2_4x) and 256 densities,
                random values, random 8-bit mixture weights over en-us's mdef
"""
from __future__ import annotations

import json
import os
import shutil
import struct
import zlib

import numpy as np

from soundswallower_amd.synth import lcg_uniform

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EN_US = os.path.join(ROOT, "soundswallower_amd", "model", "en-us")
MODEL_A = os.path.join(GOLD, "sc", "en-us-cb41")
FEAT_A = os.path.join(GOLD, "sc", "goforward_feat.npy")
RESULTS_JSON = os.path.join(GOLD, "sc_results.json")
ROWS_NPZ = os.path.join(GOLD, "sc", "rows.npz")  # the whole rows of sc_results.json, int16
CUT_CODEBOOK = 41
TIES = ((9, (10, 40, 41, 42, 100)), (3, (2,)))
B_VECLEN = (12, 24, 3, 12)
B_DENSITIES = 256
B_SEED = 20261019
B_FRAMES = 64
SETTINGS = ((1, 1), (2, 1), (3, 1), (4, 2), (4, 3))  # (topn, ds) recorded for model A
INT32_MIN = -(1 << 31)
# the model files every single-codebook test model shares with en-us, used by path
SHARED = ("mdef", "transition_matrices", "dict.txt", "noisedict.txt")


# ------------------------------------------------------------------------------------------
# s3 files
# ------------------------------------------------------------------------------------------
def write_s3(path, payload):
    """payload (whole 32-bit words) under an s3 header with its checksum (the reference reads
    the trailing checksum word whatever the header says)"""
    hdr = b"s3\nversion 1.0\nchksum0 yes\nendhdr\n"
    s = 0
    for w in np.frombuffer(payload, "<u4").tolist():
        s = (((s << 20) | (s >> 12)) + w) & 0xFFFFFFFF
    with open(path, "wb") as fh:
        fh.write(hdr + struct.pack("<I", 0x11223344) + payload + struct.pack("<I", s))


def read_gauss(path):
    """(n_cb, veclen tuple, [stream] float32 [n_cb][n_density][veclen_f]) of a means / variances
    file (file order is [cb][stream][density][veclen])"""
    with open(path, "rb") as fh:
        blob = fh.read()
    end = blob.index(b"endhdr\n") + len(b"endhdr\n")
    assert struct.unpack_from("<I", blob, end)[0] == 0x11223344
    n_cb, n_feat, n_den = struct.unpack_from("<3i", blob, end + 4)
    vl = struct.unpack_from("<%di" % n_feat, blob, end + 16)
    n = struct.unpack_from("<i", blob, end + 16 + 4 * n_feat)[0]
    data = np.frombuffer(blob, "<f4", n, end + 20 + 4 * n_feat)
    per_cb = n_den * sum(vl)
    streams, at = [], 0
    for v in vl:
        cols = [data[c * per_cb + at:c * per_cb + at + n_den * v].reshape(n_den, v)
                for c in range(n_cb)]
        streams.append(np.stack(cols).astype(np.float32))
        at += n_den * v
    return n_cb, tuple(vl), streams


def write_gauss(path, streams):
    """streams: [stream] float32 [n_cb][n_density][veclen_f]"""
    n_cb, n_den = streams[0].shape[:2]
    vl = [s.shape[2] for s in streams]
    body = b"".join(np.ascontiguousarray(s[c], "<f4").tobytes()
                    for c in range(n_cb) for s in streams)
    write_s3(path, struct.pack("<3i", n_cb, len(streams), n_den) + struct.pack("<%di" % len(vl), *vl)
             + struct.pack("<i", len(body) // 4) + body)


def _dump_str(s):
    b = s.encode() + b"\0"
    return struct.pack("<i", len(b)) + b


def write_sendump8(path, mixw):
    """mixw uint8 [n_feat][n_density][n_sen] as an unclustered 8-bit sendump, bytes as given"""
    n_feat, n_den, n_sen = mixw.shape
    out = _dump_str("sendump of a test model") + _dump_str("8-bit mixture weights")
    for kv in ("feature_count %d" % n_feat, "mixture_count %d" % n_den, "model_count %d" % n_sen):
        out += _dump_str(kv)
    out += struct.pack("<i", 0) + struct.pack("<2i", n_den, n_sen)
    with open(path, "wb") as fh:
        fh.write(out + np.ascontiguousarray(mixw, np.uint8).tobytes())


def write_sendump4(path, codebook, codes):
    """codes uint8 [n_feat][n_density][n_sen] (0..15) into a 4-bit clustered sendump: senone j's
    code in the low nibble of byte j / 2 when j is even, in the high nibble when it is odd"""
    n_feat, n_den, n_sen = codes.shape
    assert len(codebook) == 16
    out = _dump_str("sendump of a test model") + _dump_str("4-bit clustered mixture weights")
    for kv in ("feature_count %d" % n_feat, "mixture_count %d" % n_den, "model_count %d" % n_sen,
               "cluster_count 16", "cluster_bits 4"):
        out += _dump_str(kv)
    out += struct.pack("<i", 0) + bytes(bytearray(int(x) for x in codebook))
    c = np.zeros((n_feat, n_den, (n_sen + 1) // 2 * 2), np.uint8)
    c[:, :, :n_sen] = codes
    packed = (c[:, :, 0::2] | (c[:, :, 1::2] << 4)).astype(np.uint8)
    with open(path, "wb") as fh:
        fh.write(out + packed.tobytes())


def read_sendump8(path):
    """uint8 [n_feat][n_density][n_sen] of an unclustered 8-bit sendump"""
    with open(path, "rb") as fh:
        blob = fh.read()
    at, kv = 0, {}
    for i in range(1000):
        n = struct.unpack_from("<i", blob, at)[0]
        at += 4
        if n == 0:
            break
        s = blob[at:at + n - 1].decode("latin-1")
        at += n
        if i >= 2 and " " in s:
            k, _, v = s.partition(" ")
            kv[k] = v
    assert int(kv.get("cluster_count", "0")) == 0
    rows, cols = struct.unpack_from("<2i", blob, at)
    at += 8
    n_feat = int(kv["feature_count"])
    return np.frombuffer(blob, np.uint8, n_feat * rows * cols, at).reshape(n_feat, rows, cols)


# ------------------------------------------------------------------------------------------
# the models
# ------------------------------------------------------------------------------------------
def cut_codebook(src, dst, cb=CUT_CODEBOOK):
    """means / variances of `src` with codebook `cb` alone, written to `dst`"""
    _, _, streams = read_gauss(src)
    write_gauss(dst, [s[cb:cb + 1] for s in streams])


def _link_shared(d, names=SHARED):
    for n in names:
        shutil.copyfile(os.path.join(EN_US, n), os.path.join(d, n))


def model_a_dir(d):
    """a directory laid out like a model's from the committed cut and en-us's other files"""
    os.makedirs(d, exist_ok=True)
    _link_shared(d, SHARED + ("sendump",))
    for n in ("means", "variances", "feat_params.json"):
        shutil.copyfile(os.path.join(MODEL_A, n), os.path.join(d, n))
    return d


def model_a_ties_dir(d):
    os.makedirs(d, exist_ok=True)
    _link_shared(d, SHARED + ("sendump",))
    shutil.copyfile(os.path.join(MODEL_A, "feat_params.json"), os.path.join(d, "feat_params.json"))
    for n in ("means", "variances"):
        _, _, streams = read_gauss(os.path.join(MODEL_A, n))
        for s in streams:
            for src, dsts in TIES:
                for k in dsts:
                    s[0, k] = s[0, src]
        write_gauss(os.path.join(d, n), streams)
    return d


def model_b_tables(seed=B_SEED, n_sen=5126):
    """(means, variances: [stream] float32 [1][256][veclen]; mixw uint8 [4][256][n_sen])"""
    tot = B_DENSITIES * sum(B_VECLEN)
    u = lcg_uniform(seed, 2 * tot)
    means, variances, at = [], [], 0
    for v in B_VECLEN:
        k = B_DENSITIES * v
        means.append((u[at:at + k] * 2.0 - 1.0).astype(np.float32).reshape(1, B_DENSITIES, v))
        variances.append((0.5 + 1.5 * u[tot + at:tot + at + k]).astype(np.float32)
                         .reshape(1, B_DENSITIES, v))
        at += k
    w = lcg_uniform(seed + 1, len(B_VECLEN) * B_DENSITIES * n_sen)
    mixw = np.floor(w * 160.0).astype(np.uint8).reshape(len(B_VECLEN), B_DENSITIES, n_sen)
    return means, variances, mixw


def model_b_dir(d, seed=B_SEED):
    os.makedirs(d, exist_ok=True)
    _link_shared(d)
    means, variances, mixw = model_b_tables(seed)
    write_gauss(os.path.join(d, "means"), means)
    write_gauss(os.path.join(d, "variances"), variances)
    write_sendump8(os.path.join(d, "sendump"), mixw)
    with open(os.path.join(MODEL_A, "feat_params.json"), encoding="utf-8") as fh:
        fp = json.load(fh)
    fp["feat"] = "s2_4x"
    fp.pop("svspec", None)
    with open(os.path.join(d, "feat_params.json"), "w", encoding="utf-8") as fh:
        json.dump(fp, fh, indent=0)
        fh.write("\n")
    return d


def model_b_features(means, n_frames=B_FRAMES, seed=B_SEED + 2):
    """rows near the means, as synth_features draws them: per stream a density, then
    x = mean + (u - 0.5) * 0.5; float32 [n_frames][51]"""
    per = sum(1 + v for v in B_VECLEN)
    u = lcg_uniform(seed, n_frames * per).reshape(n_frames, per)
    out = np.empty((n_frames, sum(B_VECLEN)), np.float32)
    at = col = 0
    for f, v in enumerate(B_VECLEN):
        cw = np.floor(u[:, at] * B_DENSITIES).astype(np.int64)
        noise = ((u[:, at + 1:at + 1 + v] - 0.5) * 0.5).astype(np.float32)
        out[:, col:col + v] = (means[f][0, cw, :] + noise).astype(np.float32)
        at += 1 + v
        col += v
    return out


def model_paths(d):
    return dict(mdef=os.path.join(d, "mdef"), means=os.path.join(d, "means"),
                variances=os.path.join(d, "variances"), sendump=os.path.join(d, "sendump"),
                tmat=os.path.join(d, "transition_matrices"))


# ------------------------------------------------------------------------------------------
# the scorer, restated
# ------------------------------------------------------------------------------------------
def _trunc(d):
    """(int32)d, INT32_MIN below the int range"""
    return INT32_MIN if d < np.float32(-2147483648.0) else int(d)


class Restated:
    """s2_semi over host tables: det float32 [n_feat][n_density]; mean, var (the SCALED
    variances, 1 / (2 var) in log units) [stream] float32 [n_density][veclen_f]; mixw uint8
    [n_feat][n_density][n_sen]; logadd uint8 [256]"""

    def __init__(self, mean, var, det, mixw, logadd, topn=4, ds=1):
        self.mean, self.var, self.det, self.mixw = mean, var, det, mixw
        self.tab = np.zeros(1024, np.int32)
        self.tab[:len(logadd)] = logadd
        self.topn, self.ds = topn, ds
        self.ptm_rule = False  # True: ptm_mgau's accept rule instead, to show that it differs
        self.n_feat = len(mean)
        self.off = np.concatenate([[0], np.cumsum([m.shape[1] for m in mean])]).astype(int)
        self.reset()

    def reset(self):
        """the ring of two slots as s2_semi_mgau_init leaves it: codeword k, worst score"""
        self.hist = [[[[k, INT32_MIN] for k in range(self.topn)] for _ in range(self.n_feat)]
                     for _ in range(2)]

    def slot_codewords(self, slot):
        return [[e[0] for e in self.hist[slot][f]] for f in range(self.n_feat)]

    def _partials(self, f, x):
        """[n_density][veclen + 1]: d after 0, 1, .. veclen dimensions, unfused float32"""
        mean, var = self.mean[f], self.var[f]
        p = np.empty((mean.shape[0], mean.shape[1] + 1), np.float32)
        p[:, 0] = self.det[f]
        for j in range(mean.shape[1]):
            diff = (x[j] - mean[:, j]).astype(np.float32)
            sq = (diff * diff).astype(np.float32)
            p[:, j + 1] = (p[:, j] - (sq * var[:, j]).astype(np.float32)).astype(np.float32)
        return p

    def frame(self, t, x):
        """frame number t of its utterance, feature row x: the int16 senone row"""
        cur, prev = self.hist[t % 2], self.hist[(t + 1) % 2]
        row = np.zeros(self.mixw.shape[2], np.int16)
        for f in range(self.n_feat):
            lst = [list(e) for e in prev[f]]
            p = self._partials(f, x[self.off[f]:self.off[f + 1]])
            vl = p.shape[1] - 1
            # eval_topn: re-score last frame's codewords, insertion with strict >
            for i in range(self.topn):
                lst[i][1] = _trunc(p[lst[i][0], vl])
                e, j = lst[i], i - 1
                while j >= 0 and e[1] > lst[j][1]:
                    lst[j + 1] = lst[j]
                    j -= 1
                lst[j + 1] = e
            if t % self.ds == 0:
                # eval_cb: every density in index order, the worst entry read live
                for cw in range(p.shape[0]):
                    worst = lst[-1][1]
                    if not bool(np.all(p[cw, :vl] >= np.float32(worst))):
                        continue  # a test before one of the dimensions failed
                    if self.ptm_rule and not p[cw, vl] >= np.float32(worst):
                        continue  # (PTM tests the final sum too: test_sc_fixture.py)
                    d_int = _trunc(p[cw, vl])
                    if d_int < worst or any(e[0] == cw for e in lst):
                        continue
                    j = self.topn - 2
                    while j >= 0 and d_int >= lst[j][1]:
                        lst[j + 1] = lst[j]
                        j -= 1
                    lst[j + 1] = [cw, d_int]
            # mgau_norm, topn_beam = 0
            norm = lst[0][1] >> 10
            for e in lst:
                e[1] = min(96, -((e[1] >> 10) - norm))
            cur[f] = lst
            # get_scores_8b_feat_all
            tmp = self.mixw[f][lst[0][0]].astype(np.int32) + lst[0][1]
            for k in range(1, self.topn):
                y = self.mixw[f][lst[k][0]].astype(np.int32) + lst[k][1]
                hi, lo = np.maximum(tmp, y), np.minimum(tmp, y)
                tmp = lo - self.tab[hi - lo]
            row = (row.astype(np.int32) + tmp).astype(np.int16)
        return row

    def utterance(self, feats):
        """rows of one utterance, frames numbered from 0, from the ring as it stands"""
        return np.stack([self.frame(t, feats[t]) for t in range(len(feats))]) if len(feats) \
            else np.zeros((0, self.mixw.shape[2]), np.int16)


def restated_from_model(model, topn=4, ds=1):
    """a Restated over the host tables of a loaded soundswallower_amd.Model"""
    vl = [int(v) for v in model.veclen]
    nd = model.n_density
    mean = model.table("mean")
    var = model.table("var")
    det = model.table("det").reshape(len(vl), nd)
    ms, vs, at = [], [], 0
    for v in vl:
        ms.append(mean[at:at + nd * v].reshape(nd, v).copy())
        vs.append(var[at:at + nd * v].reshape(nd, v).copy())
        at += nd * v
    mixw = model.table("ptm_mixw").reshape(len(vl), nd, model.n_sen)
    return Restated(ms, vs, det, mixw, model.table("logadd8"), topn, ds)


def row_crcs(rows):
    return [zlib.crc32(np.ascontiguousarray(r, "<i2").tobytes()) & 0xFFFFFFFF for r in rows]


def split_rows(got):
    """(the results without their whole rows -- `rows` keeps the frame numbers --, {case/frame:
    int16 row}): how the fixture is stored, the rows as a compressed binary file"""
    rows = {}
    for case, rec in got["scoring"].items():
        for t, row in rec["rows"].items():
            rows["%s/%s" % (case, t)] = np.array(row, np.int16)
        rec["rows"] = sorted(rec["rows"], key=int)
    return got, rows


def results():
    """the fixture, the whole rows back in place: scoring.<case>.rows = {frame: [n_sen]}"""
    with open(RESULTS_JSON, encoding="utf-8") as fh:
        fx = json.load(fh)
    with np.load(ROWS_NPZ) as z:
        for case, rec in fx["scoring"].items():
            rec["rows"] = {t: z["%s/%s" % (case, t)].tolist() for t in rec["rows"]}
    return fx


# ------------------------------------------------------------------------------------------
# models the loader has to refuse
# ------------------------------------------------------------------------------------------
def _random_gauss(d, n_cb, n_density, veclen, seed):
    k = n_cb * n_density * sum(veclen)
    u = lcg_uniform(seed, 2 * k)
    means, variances, at = [], [], 0
    for v in veclen:
        n = n_cb * n_density * v
        means.append((u[at:at + n] * 2.0 - 1.0).astype(np.float32).reshape(n_cb, n_density, v))
        variances.append((0.5 + 1.5 * u[k + at:k + at + n]).astype(np.float32)
                         .reshape(n_cb, n_density, v))
        at += n
    os.makedirs(d, exist_ok=True)
    _link_shared(d, ("mdef", "transition_matrices"))
    write_gauss(os.path.join(d, "means"), means)
    write_gauss(os.path.join(d, "variances"), variances)
    # (a sendump of the right shape: the refusals below come before it is read, and a loader
    # that got that far would not stumble over a missing file instead)
    write_sendump8(os.path.join(d, "sendump"),
                   np.zeros((len(veclen), n_density, 5126), np.uint8))
    return d


def refused_models(tmp):
    """{name: (directory, topn, words the refusal has to hold)}: what the loader must refuse,
    naming the scorer and the limit (the last one: the PTM records' limit, 42 codebooks)"""
    a = model_a_dir(os.path.join(tmp, "refused_topn5"))
    return {
        "topn5": (a, 5, ("s2_semi", "topn 5")),
        "257_densities": (_random_gauss(os.path.join(tmp, "refused_257"), 1, 257, (13, 13, 13), 7),
                          4, ("s2_semi", "257 densities")),
        "33_dimensions": (_random_gauss(os.path.join(tmp, "refused_33"), 1, 8, (12, 33), 8),
                          4, ("s2_semi", "33 dimensions")),
        "20_dimensions_42_codebooks": (_random_gauss(os.path.join(tmp, "refused_20"), 42, 4, (20,), 9),
                                       4, ("20 dimensions",)),
    }
