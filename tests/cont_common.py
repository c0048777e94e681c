"""Continuous-density (one codebook per senone) test models and a plain restatement of the ms
scorer on them.

The builders make the models of the continuous tests deterministically from the en-us files in
the tree, into a directory the caller names (nothing of their size is committed); score()
restates compute_dist (src/ms_gauden.c:349-432), senone_eval (src/ms_senone.c:314-362) and
ms_cont_mgau_frame_eval with compallsen = yes (src/ms_mgau.c:299-321) with the reference's own
loops -- the early exit, the insertion, the log-add chain -- in numpy float32 / int32, every
senone (and frame) of a step at once.

  C3        5126 codebooks, 3 streams x 13, K = 8 densities: for senone s and stream f the 8
            densities of en-us codebook sen2cimap[s] whose PTM mixture weight for s is smallest
            (ties to the lower index), in index order; weights logbase^-(q << 10)
  C1        one stream of 39 (feat_params.json without svspec), 6 densities: density k is the
            concatenation of C3's k-th density of the three streams, its weight their product
  C3-ties   C3 with density 2 copied over density 6 in every codebook (means and variances; the
            weights stay): every (frame, senone, stream) has an exact tie
  synthetic seeded random files of any shape, loaded without an mdef
"""
from __future__ import annotations

import json
import os
import shutil
import struct
import zlib

import numpy as np

from soundswallower_amd.synth import lcg_uniform
from tests import sc_common as S

ROOT = S.ROOT
GOLD = S.GOLD
EN_US = S.EN_US
RESULTS_JSON = os.path.join(GOLD, "cont_results.json")
ROWS_NPZ = os.path.join(GOLD, "cont", "rows.npz")
K = 8             # densities of C3
C1_DENSITIES = 6
TIE = (2, 6)      # C3-ties: density 2 copied over density 6
LOGBASE = 1.0001
INT32_MIN = -(1 << 31)
WORST_DIST = np.float32(-2147483648.0)
SHARED = ("mdef", "transition_matrices", "dict.txt", "noisedict.txt")
# scoring cases recorded from the reference: name -> (model, topn, aw, mixwfloor, feature scale)
CASES = {
    "C3": ("C3", 4, 1, 1e-7, 1),
    "C3_topn1": ("C3", 1, 1, 1e-7, 1),
    "C3_topn2": ("C3", 2, 1, 1e-7, 1),
    "C3_topn8": ("C3", 8, 1, 1e-7, 1),
    "C3_aw2": ("C3", 4, 2, 1e-7, 1),
    "C3_mixwfloor": ("C3", 4, 1, 1e-3, 1),
    "C3_scaled": ("C3", 4, 1, 1e-7, 40),
    "C3-ties": ("C3-ties", 4, 1, 1e-7, 1),
    "C1": ("C1", 4, 1, 1e-7, 1),
    "C1_topn0": ("C1", 0, 1, 1e-7, 1),
    "C1_topn6": ("C1", 6, 1, 1e-7, 1),
}


# ------------------------------------------------------------------------------------------
# files
# ------------------------------------------------------------------------------------------
def write_mixw(path, w):
    """w float32 [n_sen][n_feat][n_density] as an s3 mixture_weights file"""
    n_sen, n_feat, n_den = w.shape
    body = np.ascontiguousarray(w, "<f4").tobytes()
    S.write_s3(path, struct.pack("<4i", n_sen, n_feat, n_den, n_sen * n_feat * n_den) + body)


def _en_us_tables():
    """(sen2cimap int [n_sen], ptm mixture weights uint8 [3][128][n_sen]) of en-us"""
    import soundswallower_amd as ssw
    m = ssw.Model(EN_US, config={"device": ssw.SSW_DEVICE_NONE})
    s2c = m.table("sen2cb").astype(np.int64)
    q = m.table("ptm_mixw").reshape(m.n_feat, m.n_density, m.n_sen)
    m.close()
    return s2c, q


_C3_CACHE = {}


def c3_tables(k=K):
    """([stream] means, [stream] variances: float32 [n_sen][k][13]; weights float32 [n_sen][3][k])"""
    if k not in _C3_CACHE:
        s2c, q = _en_us_tables()
        _, _, mean = S.read_gauss(os.path.join(EN_US, "means"))
        _, _, var = S.read_gauss(os.path.join(EN_US, "variances"))
        n_sen = len(s2c)
        ms, vs = [], []
        w = np.zeros((n_sen, 3, k), np.float32)
        sen = np.arange(n_sen)
        for f in range(3):
            qf = q[f].T.astype(np.int64)  # [n_sen][128]
            # the k smallest values, ties to the lower index; then in index order
            pick = np.sort(np.argsort(qf, axis=1, kind="stable")[:, :k], axis=1)
            ms.append(mean[f][s2c[:, None], pick].astype(np.float32))
            vs.append(var[f][s2c[:, None], pick].astype(np.float32))
            qq = qf[sen[:, None], pick]
            w[:, f, :] = np.power(np.float64(LOGBASE), -(qq << 10).astype(np.float64)).astype(np.float32)
        _C3_CACHE[k] = (ms, vs, w)
    ms, vs, w = _C3_CACHE[k]
    return [m.copy() for m in ms], [v.copy() for v in vs], w.copy()


def _shared(d, feat_params):
    os.makedirs(d, exist_ok=True)
    for n in SHARED:
        shutil.copyfile(os.path.join(EN_US, n), os.path.join(d, n))
    with open(os.path.join(d, "feat_params.json"), "w", encoding="utf-8") as fh:
        json.dump(feat_params, fh, indent=0)
        fh.write("\n")


def _feat_params(svspec=True):
    with open(os.path.join(EN_US, "feat_params.json"), encoding="utf-8") as fh:
        fp = json.load(fh)
    if not svspec:
        fp.pop("svspec", None)
    return fp


def model_c3_dir(d, ties=False):
    ms, vs, w = c3_tables()
    if ties:
        for a in ms + vs:
            a[:, TIE[1]] = a[:, TIE[0]]
    _shared(d, _feat_params())
    S.write_gauss(os.path.join(d, "means"), ms)
    S.write_gauss(os.path.join(d, "variances"), vs)
    write_mixw(os.path.join(d, "mixture_weights"), w)
    return d


def model_c1_dir(d, n_density=C1_DENSITIES, k=K):
    """(k: the densities of the C3 tables it is made of; the timing tool makes one of 32)"""
    ms, vs, w = c3_tables(k)
    mean = np.concatenate([m[:, :n_density] for m in ms], axis=2)
    var = np.concatenate([v[:, :n_density] for v in vs], axis=2)
    w1 = ((w[:, 0, :n_density] * w[:, 1, :n_density]).astype(np.float32)
          * w[:, 2, :n_density]).astype(np.float32)
    _shared(d, _feat_params(svspec=False))
    S.write_gauss(os.path.join(d, "means"), [mean])
    S.write_gauss(os.path.join(d, "variances"), [var])
    write_mixw(os.path.join(d, "mixture_weights"), w1[:, None, :])
    return d


BUILDERS = {"C3": model_c3_dir, "C3-ties": lambda d: model_c3_dir(d, ties=True), "C1": model_c1_dir}


def model_paths(d, mdef=True):
    return dict(mdef=os.path.join(d, "mdef") if mdef else None, means=os.path.join(d, "means"),
                variances=os.path.join(d, "variances"), mixw=os.path.join(d, "mixture_weights"),
                tmat=os.path.join(d, "transition_matrices") if mdef else None)


def synthetic_dir(d, n_sen, veclen, n_density, seed, n_cb=None):
    """seeded random means, variances and mixture weights; no mdef.  n_cb: codebooks in the
    Gaussian files when they are not to number the senones (the refusals)"""
    n_cb = n_sen if n_cb is None else n_cb
    tot = n_cb * n_density * sum(veclen)
    u = lcg_uniform(seed, 2 * tot + n_sen * len(veclen) * n_density)
    ms, vs, at = [], [], 0
    for v in veclen:
        n = n_cb * n_density * v
        ms.append((u[at:at + n] * 2.0 - 1.0).astype(np.float32).reshape(n_cb, n_density, v))
        vs.append((0.5 + 1.5 * u[tot + at:tot + at + n]).astype(np.float32).reshape(n_cb, n_density, v))
        at += n
    w = (0.01 + u[2 * tot:]).astype(np.float32).reshape(n_sen, len(veclen), n_density)
    os.makedirs(d, exist_ok=True)
    S.write_gauss(os.path.join(d, "means"), ms)
    S.write_gauss(os.path.join(d, "variances"), vs)
    write_mixw(os.path.join(d, "mixture_weights"), w)
    return d


def synthetic_features(n_frames, dim, seed):
    return (lcg_uniform(seed, n_frames * dim) * 3.0 - 1.5).astype(np.float32).reshape(n_frames, dim)


# ------------------------------------------------------------------------------------------
# the scorer, restated
# ------------------------------------------------------------------------------------------
def _fden(dist):
    """senone_eval's density term (src/ms_senone.c:332-335), int32 arrays"""
    low = dist < WORST_DIST
    with np.errstate(invalid="ignore"):
        i = np.where(low, 0, dist).astype(np.int64)
    return np.where(low, INT32_MIN >> 10, (i + 1023) >> 10).astype(np.int64)


class Restated:
    """the ms scorer with the .cont. map over host tables: mean, var (the SCALED variances)
    [stream] float32 [n_sen][n_density][veclen_f]; det float32 [n_sen][n_feat][n_density]; pdf uint8
    [n_sen][n_feat][n_density]; logadd uint8 [256]"""

    def __init__(self, mean, var, det, pdf, logadd, topn, aw=1):
        self.mean, self.var, self.det, self.pdf = mean, var, det, pdf.astype(np.int64)
        self.tab = np.asarray(logadd, np.int64)
        assert len(self.tab) == 256
        self.n_density = mean[0].shape[1]
        self.topn = self.n_density if topn < 1 or topn > self.n_density else topn
        self.aw = aw
        self.zero = INT32_MIN >> 12  # logmath's zero at shift 10
        self.off = np.concatenate([[0], np.cumsum([m.shape[2] for m in mean])]).astype(int)

    def _logadd(self, x, y):
        """logmath_add (src/logmath.c:228-272) on the 8-bit table"""
        d = np.abs(x - y)
        r = np.maximum(x, y)
        v = r + np.where(d < 256, self.tab[np.minimum(d, 255)], 0)
        v = np.where(y <= self.zero, x, v)
        return np.where(x <= self.zero, y, v)

    def _dist(self, f, x):
        """compute_dist for every (frame, senone): (dist float32 [T][S][topn], id [T][S][topn])"""
        mean, var, det = self.mean[f], self.var[f], self.det[:, f, :]
        T, S_, vl, nd, n_top = x.shape[0], mean.shape[0], mean.shape[2], self.n_density, self.topn
        if n_top >= nd:  # compute_dist_all: every density in index order, no early exit
            dist = np.empty((T, S_, nd), np.float32)
            for d in range(nd):
                dval = np.broadcast_to(det[None, :, d], (T, S_)).astype(np.float32)
                for i in range(vl):
                    diff = (x[:, None, i] - mean[None, :, d, i]).astype(np.float32)
                    dval = (dval - ((diff * diff).astype(np.float32) * var[None, :, d, i])
                            .astype(np.float32)).astype(np.float32)
                dist[:, :, d] = dval
            return dist, np.broadcast_to(np.arange(nd), (T, S_, nd))
        dist = np.full((T, S_, n_top), WORST_DIST, np.float32)
        ids = np.zeros((T, S_, n_top), np.int64)
        for d in range(nd):
            worst = dist[:, :, n_top - 1]
            dval = np.broadcast_to(det[None, :, d], (T, S_)).astype(np.float32)
            going = np.ones((T, S_), bool)  # the loop condition has held so far
            for i in range(vl):
                going &= dval >= worst
                diff = (x[:, None, i] - mean[None, :, d, i]).astype(np.float32)
                step = (dval - ((diff * diff).astype(np.float32) * var[None, :, d, i])
                        .astype(np.float32)).astype(np.float32)
                dval = np.where(going, step, dval)
            take = going & ~(dval < worst)  # (i < featlen) || (dval < worst->dist): continue
            # for (i = 0; i < n_top && dval < out_dist[i].dist; i++);  the list is sorted
            pos = np.zeros((T, S_), np.int64)
            still = np.ones((T, S_), bool)
            for i in range(n_top):
                still &= dval < dist[:, :, i]
                pos += still
            for j in range(n_top - 1, 0, -1):
                mv = take & (j > pos)
                dist[:, :, j] = np.where(mv, dist[:, :, j - 1], dist[:, :, j])
                ids[:, :, j] = np.where(mv, ids[:, :, j - 1], ids[:, :, j])
            for j in range(n_top):
                put = take & (pos == j)
                dist[:, :, j] = np.where(put, dval, dist[:, :, j])
                ids[:, :, j] = np.where(put, d, ids[:, :, j])
        return dist, ids

    def score(self, feats, raw=False, unclamped=False):
        """int16 [T][n_sen] of feature rows [T][dim] (raw: before the frame's best is subtracted;
        unclamped: int64, before the division by aw and the first clamp)"""
        feats = np.asarray(feats, np.float32)
        T, S_ = feats.shape[0], self.pdf.shape[0]
        scr = np.zeros((T, S_), np.int64)
        sen = np.arange(S_)[None, :]
        for f in range(len(self.mean)):
            dist, ids = self._dist(f, feats[:, self.off[f]:self.off[f + 1]])
            fscr = _fden(dist[:, :, 0]) - self.pdf[sen, f, ids[:, :, 0]]
            for t in range(1, dist.shape[2]):
                fscr = self._logadd(fscr, _fden(dist[:, :, t]) - self.pdf[sen, f, ids[:, :, t]])
            scr -= fscr
        if unclamped:
            return scr
        scr = np.where(scr < 0, -((-scr) // self.aw), scr // self.aw)  # C division
        scr = np.clip(scr, -32768, 32767)
        if raw:
            return scr.astype(np.int16)
        best = scr.min(axis=1, keepdims=True)
        return np.clip(scr - best, -32768, 32767).astype(np.int16)


def restated_from_model(model, topn=None, aw=None):
    """a Restated over the host tables of a loaded soundswallower_amd.Model"""
    vl = [int(v) for v in model.veclen]
    nd, ns, nf = model.n_density, model.n_sen, model.n_feat
    per = nd * sum(vl)
    mean = model.table("mean").reshape(ns, per)
    var = model.table("var").reshape(ns, per)
    ms, vs, at = [], [], 0
    for v in vl:
        ms.append(mean[:, at:at + nd * v].reshape(ns, nd, v).copy())
        vs.append(var[:, at:at + nd * v].reshape(ns, nd, v).copy())
        at += nd * v
    return Restated(ms, vs, model.table("det").reshape(ns, nf, nd),
                    model.table("ms_pdf").reshape(ns, nf, nd), model.table("logadd8"),
                    model.topn if topn is None else topn, 1 if aw is None else aw)


def score_in_pieces(r, feats, piece=32):
    """Restated.score a few frames at a time (the [T][S] temporaries stay small)"""
    return np.concatenate([r.score(feats[a:a + piece]) for a in range(0, len(feats), piece)])


def row_crcs(rows):
    return [zlib.crc32(np.ascontiguousarray(r, "<i2").tobytes()) & 0xFFFFFFFF for r in rows]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def split_rows(got):
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


def features():
    """the feature rows the reference scored for goforward.raw (float32 [278][39]): en-us's front
    end, the rows the s2_semi fixtures recorded"""
    return np.load(S.FEAT_A)
