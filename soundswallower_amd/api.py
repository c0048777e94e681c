"""Host-side mirror of the reference's interfaces for the accelerated path, over the C ABI.

Names follow the reference: `Model` stands for what `acmod_load_am` loads, `PtmMgau` for the
`mgau_t` returned by `ptm_mgau_init` (its `frame_eval` is the vtable slot `acmod_score`
calls), `StateAlignSearch` for `state_align_search_init/start/step/finish`.  Everything runs on
the GPU through `libssw_amd.so`; there is no CPU path here.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import (SswAlignEntry, SswCmnState, SswConfig, SswFeatConfig, SswFeConfig,
                   SswModelInfo)

SCORER_PTM = 0
SCORER_MS = 1
SCORER_S2_SEMI = 2
SSW_DEVICE_NONE = -2
INT_MAX = 2**31 - 1

_TABLES = {
    "mean": (0, np.float32), "var": (1, np.float32), "det": (2, np.float32),
    "ptm_mixw": (3, np.uint8), "ms_pdf": (4, np.uint8), "tp": (5, np.uint8),
    "sseq": (6, np.uint16), "sen2cb": (7, np.int16), "logadd8": (8, np.uint8),
    "phone_ssid": (9, np.int32), "phone_tmat": (10, np.int32),
    "rec": (11, np.float32), "scan_rec": (12, np.float32), "scan_d0": (13, np.float32),
    "scan_exact": (14, np.uint32), "scan_rec_mfma": (15, np.float32),
    "scan_exact_mfma": (16, np.uint32), "scan_wfrag": (17, np.uint16),
}


class SswError(RuntimeError):
    pass


FE_TRANSFORMS = {"legacy": 0, "dct": 1, "htk": 2}
FE_FRAME, FE_SHIFT, FE_NCEP = 410, 160, 13


CMN_TYPES = {"none": 0, "batch": 1, "current": 1, "live": 2, "prior": 2}


class FeatConfig(SswFeatConfig):
    """ssw_feat_config_t: feat, ceplen, cmn, cmninit, varnorm, lda, ldadim, svspec."""

    def update(self, **settings) -> "FeatConfig":
        names = dict(SswFeatConfig._fields_)
        for k, v in settings.items():
            if k not in names or k == "from_file":
                raise SswError(f"unknown feature setting {k!r}")
            if k == "cmn" and isinstance(v, str):
                if v not in CMN_TYPES:
                    raise SswError(f"Unknown CMN type {v!r}")
                v = CMN_TYPES[v]
            if k == "cmninit" and v is not None and not isinstance(v, (str, bytes)):
                v = ",".join(repr(float(x)) for x in v)
            if k in ("feat", "cmninit", "lda", "svspec"):
                v = b"" if v is None else os.fsencode(v)
                if len(v) >= C.sizeof(names[k]):
                    raise SswError(f"feature setting {k!r} is too long")
            setattr(self, k, int(v) if isinstance(v, bool) else v)
        return self

    @classmethod
    def read(cls, path, **settings) -> "FeatConfig":
        """The reference's defaults, a feat_params.json's keys over them (ssw_feat_config_read),
        then `settings`."""
        L = _lib.lib()
        c = cls()
        L.ssw_feat_config_defaults(C.byref(c))
        if path is not None:
            _check(L.ssw_feat_config_read(os.fsencode(path), C.byref(c)), "ssw_feat_config_read")
        return c.update(**settings)

    def as_dict(self) -> dict:
        inv = {0: "none", 1: "batch", 2: "live"}
        return {"feat": self.feat.decode(), "ceplen": int(self.ceplen),
                "cmn": inv.get(int(self.cmn), int(self.cmn)),
                "cmninit": self.cmninit.decode() or None, "varnorm": bool(self.varnorm),
                "lda": os.fsdecode(self.lda) or None, "ldadim": int(self.ldadim),
                "svspec": self.svspec.decode() or None, "from_file": bool(self.from_file)}


def fe_frame_counts(n_samples) -> np.ndarray:
    """Frames the front end makes of utterances of n_samples samples (ssw_fe_frame_count):
    0 for none, 1 below one window, else 2 + (n - 410) // 160 (fe_end's overflow frame last)."""
    n = np.asarray(n_samples, np.int64)
    return np.where(n <= 0, 0, np.where(n < FE_FRAME, 1, 2 + (n - FE_FRAME) // FE_SHIFT))


def fe_frame_counts_at(n_samples, samprate, frate=100, wlen=0.025625) -> np.ndarray:
    """Frames the front end makes of n_samples samples at samprate Hz (ssw_fe_frame_count_ex;
    a scalar rate or one per utterance, in whole hertz): shift (int)(samprate / frate + 0.5) and
    size (int)(wlen samprate + 0.5) in float32 as fe_init computes them; 0 for none, 1 below one
    window, else the full frames and fe_end's frame of the samples left over."""
    n = np.asarray(n_samples, np.int64)
    sr = np.broadcast_to(np.asarray(samprate, np.float32), n.shape)
    shift = (sr / np.float32(frate)).astype(np.float64) + 0.5
    size = (sr * np.float32(wlen)).astype(np.float64) + 0.5
    shift, size = shift.astype(np.int64), size.astype(np.int64)
    full = 1 + (n - size) // np.maximum(shift, 1)
    rest = n - full * shift
    return np.where(n <= 0, 0, np.where(n < size, 1, full + (rest > 0)))


class FirstPassConfig(C.Structure):
    """ssw_first_pass_config_t"""
    _fields_ = [("beam", C.c_double), ("pbeam", C.c_double), ("wbeam", C.c_double),
                ("wip", C.c_double), ("pip", C.c_double), ("lw", C.c_float),
                ("silprob", C.c_float), ("fillprob", C.c_float), ("use_filler", C.c_int32),
                ("use_altpron", C.c_int32), ("two_pass_history", C.c_int32)]


FP_NODE_DTYPE = np.dtype([("senid", np.uint16, 3), ("tmat", np.int16), ("pen", np.int32),
                          ("parent", np.int32), ("flags", np.uint32), ("ci_ext", np.int32),
                          ("state", np.int32), ("to_state", np.int32), ("wid", np.int32),
                          ("ctxt", np.uint64)], align=True)
WORD_SEG_DTYPE = np.dtype([("wid", np.int32), ("start", np.int32), ("duration", np.int32),
                           ("score", np.int32)])


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):  # torch tensor
        return C.c_void_p(a.data_ptr())
    return C.c_void_p(int(a))


def _check(rv, what):
    if rv is None or (isinstance(rv, int) and rv < 0):
        raise SswError(f"{what}: {_lib.last_error()}")
    return rv


def _is_device_tensor(a) -> bool:
    return hasattr(a, "data_ptr") and bool(getattr(a, "is_cuda", False))


def _pcm_kind(pcm, pcm_format=None, who="pcm") -> str:
    """The sample type of audio handed to the front end: "i16" (ssw_fe_batch, ssw_fe_batch_ex)
    or "f32" (ssw_fe_batch_f32).  np.float32 arrays and torch.float32 device tensors are "f32";
    integer arrays and torch.int16 device tensors "i16"; a raw device pointer is "i16" unless
    pcm_format="f32".  Any other dtype raises: a float64 array would be cut to integers, a
    device tensor of another type read as something it is not.  A list must be all one kind."""
    if pcm_format not in (None, "i16", "f32"):
        raise SswError(f"{who}: unknown pcm_format {pcm_format!r} (\"i16\" or \"f32\")")
    if isinstance(pcm, (list, tuple)) and pcm and not np.isscalar(pcm[0]):
        kinds = {_pcm_kind(p, pcm_format, who) for p in pcm}
        if len(kinds) > 1:
            raise SswError(f"{who}: a list of arrays must be all int16 or all float32")
        return kinds.pop()
    if hasattr(pcm, "data_ptr"):                      # torch tensor
        name = str(pcm.dtype)
        kind = {"torch.int16": "i16", "torch.float32": "f32"}.get(name)
        if kind is None or not _is_device_tensor(pcm):
            if kind is None:
                raise SswError(f"{who}: audio of dtype {name} (torch.int16 or torch.float32)")
            return _pcm_kind(pcm.numpy(), pcm_format, who)
    elif pcm is None or isinstance(pcm, (int, C.c_void_p)):
        return pcm_format or "i16"                    # a raw device pointer
    else:
        dt = np.asarray(pcm).dtype
        if dt == np.float32:
            kind = "f32"
        elif dt.kind in "iub":
            kind = "i16"
        else:
            raise SswError(f"{who}: audio of dtype {dt} (an integer type or float32)")
    if pcm_format is not None and pcm_format != kind:
        raise SswError(f"{who}: pcm_format {pcm_format!r} given for {kind} audio")
    return kind


_PCM_DTYPE = {"i16": np.int16, "f32": np.float32}


def _pcm_concat(pcm, kind):
    """One contiguous host array of the kind's dtype, and samp_off when pcm was a list."""
    dt = _PCM_DTYPE[kind]
    samp_off = None
    if isinstance(pcm, (list, tuple)):
        samp_off = np.concatenate([[0], np.cumsum([len(p) for p in pcm])]).astype(np.int64)
        pcm = np.concatenate([np.asarray(p, dt).reshape(-1) for p in pcm]) if pcm \
            else np.zeros(0, dt)
    return np.ascontiguousarray(pcm, dt).reshape(-1), samp_off


def model_dir(name: str) -> str:
    """Path of a bundled acoustic model ("en-us", "fr-fr")."""
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "model", name)


class Mllr:
    """An MLLR speaker-adaptation transform (ssw_mllr_t, the reference's mllr_t): per stream a
    rotation A [veclen][veclen], a bias b [veclen] and a variance scale h [veclen].

        Mllr.read(path)                    the reference's text format (mllr_read)
        Mllr(A=[...], b=[...], h=[...])    one array per stream, one class
    """

    def __init__(self, A=None, b=None, h=None, *, _handle=None):
        self._L = _lib.lib()
        if _handle is not None:
            self._t = _handle
            return
        if A is None or b is None or h is None or not len(A) == len(b) == len(h):
            raise SswError("Mllr: A, b and h are needed, one array per stream each")
        As = [np.ascontiguousarray(a, np.float32) for a in A]
        bs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in b]
        hs = [np.ascontiguousarray(x, np.float32).reshape(-1) for x in h]
        for f, (a, bb, hh) in enumerate(zip(As, bs, hs)):
            if a.ndim != 2 or a.shape != (len(bb), len(bb)) or len(hh) != len(bb):
                raise SswError(f"Mllr: stream {f}: A {a.shape}, b {bb.shape} and h {hh.shape} "
                               "are not [veclen][veclen], [veclen] and [veclen]")
        made = self._create_raw(1, [len(x) for x in bs], As, bs, hs)
        self._t, made._t = made._t, None

    @classmethod
    def _create_raw(cls, n_class, veclen, A, b, h) -> "Mllr":
        """ssw_mllr_create as it is: per stream flat float32 arrays, class-major"""
        L = _lib.lib()
        veclen = np.array(veclen, np.int32)
        ptrs = lambda arrs: (C.c_void_p * len(arrs))(*[x.ctypes.data for x in arrs])
        t = L.ssw_mllr_create(int(n_class), len(veclen), _ptr(veclen), ptrs(A), ptrs(b), ptrs(h))
        if not t:
            raise SswError("ssw_mllr_create: " + _lib.last_error())
        return cls(_handle=t)

    @classmethod
    def read(cls, path) -> "Mllr":
        t = _lib.lib().ssw_mllr_read(os.fsencode(path))
        if not t:
            raise SswError("ssw_mllr_read: " + _lib.last_error())
        return cls(_handle=t)

    def _struct(self):
        return C.cast(self._t, C.POINTER(_SswMllr)).contents

    @property
    def n_class(self) -> int:
        return int(self._struct().n_class)

    @property
    def veclen(self):
        s = self._struct()
        return [int(s.veclen[f]) for f in range(s.n_feat)]

    def arrays(self, klass=0):
        """(A, b, h) of one class: lists of float32 arrays, one per stream"""
        s = self._struct()
        A, b, h = [], [], []
        for f, vl in enumerate(self.veclen):
            A.append(np.array([[s.A[f][klass][l][m] for m in range(vl)] for l in range(vl)],
                              np.float32).reshape(vl, vl))
            b.append(np.array([s.b[f][klass][l] for l in range(vl)], np.float32))
            h.append(np.array([s.h[f][klass][l] for l in range(vl)], np.float32))
        return A, b, h

    def free(self):
        if getattr(self, "_t", None):
            self._L.ssw_mllr_free(self._t)
            self._t = None

    __del__ = free


class _SswMllr(C.Structure):
    """ssw_mllr_t"""
    _fp = C.POINTER(C.c_float)
    _fields_ = [("refcnt", C.c_int), ("n_class", C.c_int), ("n_feat", C.c_int),
                ("veclen", C.POINTER(C.c_int)), ("A", C.POINTER(C.POINTER(C.POINTER(_fp)))),
                ("b", C.POINTER(C.POINTER(_fp))), ("h", C.POINTER(C.POINTER(_fp))),
                ("cb2mllr", C.POINTER(C.c_int32))]


class Model:
    """Acoustic model tables on the GPU (ssw_model_load).  mllr: the path of an MLLR transform
    file, applied after the load (the reference's `mllr` configuration key).  active=True:
    enable_active() after the load (a continuous model then serves the active=True calls)."""

    def __init__(self, path=None, *, mdef=None, means=None, variances=None, sendump=None,
                 mixw=None, tmat=None, config=None, mllr=None, active=False):
        L = _lib.lib()
        if path is not None:
            j = lambda n: os.path.join(path, n)
            mdef = mdef or j("mdef")
            means = means or j("means")
            variances = variances or j("variances")
            tmat = tmat or j("transition_matrices")
            if sendump is None and mixw is None:
                if os.path.exists(j("sendump")):
                    sendump = j("sendump")
                else:
                    mixw = j("mixture_weights")
        cfg = SswConfig()
        L.ssw_config_defaults(C.byref(cfg))
        for k, v in (config or {}).items():
            setattr(cfg, k, v)
        enc = lambda s: None if s is None else os.fsencode(s)
        self._L = L
        self._m = L.ssw_model_load(enc(mdef), enc(means), enc(variances), enc(sendump),
                                   enc(mixw), enc(tmat), C.byref(cfg))
        if not self._m:
            raise SswError("ssw_model_load: " + _lib.last_error())
        self._read_info()
        # outcome of the matrix-core self-test at load (ssw_amd.h, ssw_model_info_t)
        self.selftest_message = (L.ssw_model_selftest_message(self._m) or b"").decode()
        if active:
            try:
                self.enable_active()
            except SswError:
                self.close()
                raise
        if mllr is not None:
            t = Mllr.read(mllr)
            try:
                self.apply_mllr(t)
            except SswError:
                self.close()
                raise
            finally:
                t.free()

    def _read_info(self):
        info = SswModelInfo()
        self._L.ssw_model_info(self._m, C.byref(info))
        self.info = info
        for name, ctype in SswModelInfo._fields_:
            if name != "veclen":
                setattr(self, name, float(getattr(info, name)) if ctype is C.c_float
                        else int(getattr(info, name)))
        self.veclen = [int(info.veclen[i]) for i in range(self.n_feat)]

    def apply_mllr(self, mllr):
        """ssw_model_apply_mllr, in place: the transform's class 0 on the means and variances as
        the files hold them (never on top of an earlier transform), every derived table rebuilt
        and uploaded.  None puts the files' parameters back.  A transform that does not fit the
        model is refused (SswError) and the model stays as it was."""
        _check(self._L.ssw_model_apply_mllr(self._m, None if mllr is None else mllr._t),
               "ssw_model_apply_mllr")
        self._read_info()  # (n_floored follows the variances)

    def mllr_timing(self):
        """(host ms, upload ms) of the last apply_mllr (ssw_model_mllr_timing)"""
        ms = np.zeros(2, np.float32)
        _check(self._L.ssw_model_mllr_timing(self._m, _ptr(ms)), "ssw_model_mllr_timing")
        return float(ms[0]), float(ms[1])

    @property
    def mllr_generation(self) -> int:
        """0 after load, +1 per apply_mllr that succeeded"""
        return int(self._L.ssw_model_mllr_generation(self._m))

    def close(self):
        if getattr(self, "_m", None):
            if getattr(self, "_feat0", None) is not None:
                self._feat0.free()
                self._feat0 = None
            if getattr(self, "_fe0", None) is not None:
                self._fe0.free()
                self._fe0 = None
            self._L.ssw_model_free(self._m)
            self._m = None

    __del__ = close

    def scorer(self) -> int:
        """ssw_model_scorer: the scorer the reference's acmod_load_am would choose for the model
        (SCORER_PTM, SCORER_S2_SEMI for a single codebook, SCORER_MS), -1 when it has the
        mixture weights of none."""
        return int(self._L.ssw_model_scorer(self._m))

    def pick_scorer(self, scorer=None) -> int:
        """the scorer a call without one takes: SCORER_S2_SEMI for a single-codebook model,
        SCORER_MS for a continuous one, else SCORER_PTM (where SCORER_MS is asked for by name)"""
        if scorer is not None:
            return int(scorer)
        if getattr(self, "_default_scorer", None) is None:
            self._default_scorer = (SCORER_S2_SEMI if self.scorer() == SCORER_S2_SEMI
                                    else SCORER_MS if self.continuous else SCORER_PTM)
        return self._default_scorer

    @property
    def continuous(self) -> bool:
        """ssw_model_is_continuous: one codebook per senone (the reference's `.cont.` map); the
        model is scored with SCORER_MS, in whole rows."""
        return bool(self._L.ssw_model_is_continuous(self._m))

    def enable_active(self):
        """ssw_model_enable_active: a continuous model gets the second (senone-major) Gaussian
        table of the listed-senone kernel, which doubles the Gaussians' device memory; from then
        on the active=True calls and the *_active functions take it (the reference's default
        compallsen = no).  Idempotent; nothing to do for any other model."""
        _check(self._L.ssw_model_enable_active(self._m), "ssw_model_enable_active")

    @property
    def active_enabled(self) -> bool:
        """ssw_model_active_enabled: a continuous model after enable_active()"""
        return bool(self._L.ssw_model_active_enabled(self._m))

    @property
    def tmat_n_emit(self) -> int:
        """Emitting states of the transition matrices (3 for both shipped models; 1, 2, 4 or 5
        take hmm_vit_eval's other branches, viterbi_align_any_kernel)."""
        if getattr(self, "_tmat_ne", None) is None:
            per = self.table("tp").size // max(self.n_tmat, 1)       # ne * (ne + 1) bytes a matrix
            self._tmat_ne = next((ne for ne in range(1, 17) if ne * (ne + 1) == per), 3)
        return self._tmat_ne

    def table(self, name: str) -> np.ndarray:
        """Host copy of a derived table (flat), for loader parity checks."""
        which, dtype = _TABLES[name]
        n = C.c_size_t(0)
        p = self._L.ssw_model_table(self._m, which, C.byref(n))
        if not p or n.value == 0:
            return np.zeros(0, dtype)
        buf = (C.c_char * n.value).from_address(p)
        return np.frombuffer(buf, dtype=dtype).copy()

    # ---- scoring ------------------------------------------------------------------
    def score_batch(self, feats, utt_off=None, scorer=None, out=None) -> np.ndarray:
        """Score host features [n_frames][39]; returns int16 [n_frames][n_sen] (`out`, if given:
        a caller that scores batch after batch reuses one buffer instead of faulting in 10 KB
        of fresh pages per frame)."""
        feats = np.ascontiguousarray(feats, dtype=np.float32).reshape(-1, self.veclen_total)
        n = feats.shape[0]
        off = (np.array([0, n], np.int32) if utt_off is None
               else np.ascontiguousarray(utt_off, np.int32))
        if out is None:
            out = np.zeros((n, self.n_sen), np.int16)
        assert out.dtype == np.int16 and out.shape == (n, self.n_sen) and out.flags.c_contiguous
        _check(self._L.ssw_score_batch_host(self._m, self.pick_scorer(scorer), _ptr(feats), n, _ptr(off),
                                            len(off) - 1, _ptr(out)), "ssw_score_batch_host")
        return out

    def score_batch_device(self, d_feats, n_frames, utt_off, d_out, stream=None,
                           scorer=None, share_device=False):
        """Device pointers (ints or torch tensors); asynchronous on `stream`.  share_device:
        SSW_SCORE_SHARE_DEVICE, for callers that run another stream's kernels beside it."""
        off = np.ascontiguousarray(utt_off, np.int32)
        st = C.c_void_p(int(stream)) if stream else None
        if share_device:
            _check(self._L.ssw_score_batch_ex(self._m, self.pick_scorer(scorer), _ptr(d_feats), int(n_frames),
                                              _ptr(off), len(off) - 1, _ptr(d_out), st, 2, None,
                                              None), "ssw_score_batch_ex")
            return
        _check(self._L.ssw_score_batch(self._m, self.pick_scorer(scorer), _ptr(d_feats), int(n_frames), _ptr(off),
                                       len(off) - 1, _ptr(d_out), st),
               "ssw_score_batch")

    def score_batch_carry(self, feats, utt_off=None, carry_in=None, carry_utts=False,
                          scorer=None, rewind=False):
        """ssw_score_batch_ex on host features: returns (scores int16 [n][n_sen], carry_out
        uint32 [n_cb * n_feat]); carry_in = the carry_out of an earlier call (or None).
        rewind = SSW_SCORE_CARRY_OUT_REWIND: carry_out is what the NEXT utterance, or the second
        pass over this one after acmod_rewind, starts from (history slot 1 of the reference's
        ring) instead of what a continuation of the same utterance starts from."""
        feats = np.ascontiguousarray(feats, dtype=np.float32).reshape(-1, self.veclen_total)
        n = feats.shape[0]
        off = (np.array([0, n], np.int32) if utt_off is None
               else np.ascontiguousarray(utt_off, np.int32))
        out = np.zeros((n, self.n_sen), np.int16)
        cin = None if carry_in is None else np.ascontiguousarray(carry_in, np.uint32)
        cout = np.zeros(self.n_cb * self.n_feat, np.uint32)
        if n == 0:
            return out, (cin.copy() if cin is not None else np.full_like(cout, 0x03020100))
        flags = (1 if carry_utts else 0) | (4 if rewind else 0)
        d_in = self.to_device(feats)
        d_out = self.device_malloc(out.nbytes)
        try:
            _check(self._L.ssw_score_batch_ex(self._m, self.pick_scorer(scorer), d_in, n, _ptr(off), len(off) - 1,
                                              d_out, None, flags, _ptr(cin),
                                              _ptr(cout)), "ssw_score_batch_ex")
            _check(self._L.ssw_memcpy_d2h(_ptr(out), d_out, out.nbytes), "ssw_memcpy_d2h")
        finally:
            self.device_free(d_in)
            self.device_free(d_out)
        return out, cout

    def last_topn(self, n_frames):
        n_cbf = self.n_cb * self.n_feat
        cw = np.zeros((n_frames, self.n_cb, self.n_feat, self.topn), np.uint8)
        sc = np.zeros((n_frames, self.n_cb, self.n_feat, self.topn), np.int32)
        _check(self._L.ssw_score_batch_topn(self._m, n_frames, _ptr(cw), _ptr(sc)),
               "ssw_score_batch_topn")
        assert cw.size == n_frames * n_cbf * self.topn
        return cw, sc

    def debug_mfma_f16_tiles(self, A, B, C):
        """D = A B + C per tile on the matrix cores (one v_mfma_f32_32x32x16_f16 each):
        A float16 [n][32][16], B float16 [n][16][32], C float32 [n][32][32]."""
        A = np.ascontiguousarray(A, np.float16)
        B = np.ascontiguousarray(B, np.float16)
        C = np.ascontiguousarray(C, np.float32)
        n = len(A)
        assert A.shape == (n, 32, 16) and B.shape == (n, 16, 32) and C.shape == (n, 32, 32)
        D = np.zeros_like(C)
        _check(self._L.ssw_debug_mfma_f16_tiles(self._m, _ptr(A), _ptr(B), _ptr(C), _ptr(D), n),
               "ssw_debug_mfma_f16_tiles")
        return D

    def debug_scan_keys(self, feats, cbf):
        """Raw keys of the matrix-core scan for one codebook x stream: float32 [n_frames][128]."""
        feats = np.ascontiguousarray(feats, np.float32).reshape(-1, self.veclen_total)
        d = self.to_device(feats)
        out = np.zeros((len(feats), 128), np.float32)
        try:
            _check(self._L.ssw_debug_scan_keys(self._m, d, len(feats), int(cbf), _ptr(out)),
                   "ssw_debug_scan_keys")
        finally:
            self.device_free(d)
        return out

    def debug_scan_top5(self, keys):
        """The scan's selection on caller-supplied keys float32 [n_frames][128]: (densities
        int32 [n_frames][5], best first; their keys with the 7 label bits cleared)."""
        if not hasattr(self._L, "ssw_debug_scan_top5"):
            raise RuntimeError("the loaded libssw_amd.so has no ssw_debug_scan_top5 "
                               "(an older build loaded through SSW_AMD_LIB?)")
        keys = np.ascontiguousarray(keys, np.float32)
        assert keys.ndim == 2 and keys.shape[1] == 128
        idx = np.zeros((len(keys), 5), np.int32)
        top = np.zeros((len(keys), 5), np.float32)
        _check(self._L.ssw_debug_scan_top5(self._m, _ptr(keys), len(keys), _ptr(idx), _ptr(top)),
               "ssw_debug_scan_top5")
        return idx, top

    def set_kernel_timing(self, enable=True):
        _check(self._L.ssw_set_kernel_timing(self._m, int(bool(enable))), "ssw_set_kernel_timing")

    def kernel_timing(self):
        """(topn_ms, senone_ms) of the last score_batch call, from HIP events on its stream.  For
        a batch scored in pieces (no split exists) the first number is the whole call and the
        second 0; `self.timing_split` says which it was."""
        ms = np.zeros(2, np.float32)
        n = _check(self._L.ssw_get_kernel_timing(self._m, _ptr(ms), 2), "ssw_get_kernel_timing")
        self.timing_split = n == 2
        return float(ms[0]), float(ms[1])

    def last_stats(self):
        st = np.zeros(2, np.int64)
        self._L.ssw_score_batch_stats(self._m, _ptr(st))
        return int(st[0]), int(st[1])

    def scan_audit_stats(self):
        """SSW_SCAN_AUDIT=k: (proven pairs redone exactly by audited waves, of those the pairs
        whose exact result differs from the scan's), running totals since the model was loaded."""
        st = np.zeros(2, np.int64)
        self._L.ssw_scan_audit_stats(self._m, _ptr(st))
        return int(st[0]), int(st[1])

    def align_stats(self):
        """(utterances through the byte-token alignment kernel, of those handed on to the
        full-token kernel), running totals"""
        st = np.zeros(2, np.int64)
        self._L.ssw_align_stats(self._m, _ptr(st))
        return int(st[0]), int(st[1])

    def first_pass_active_stats(self):
        """ssw_first_pass_active_stats: (utterances searched in the default configuration as a
        batch, their rounds summed, rounds of the last call, utterances that needed more than
        one round), running totals"""
        st = np.zeros(4, np.int64)
        self._L.ssw_first_pass_active_stats(self._m, _ptr(st))
        return tuple(int(x) for x in st)

    def grammar_active_stats(self):
        """ssw_grammar_active_stats: first_pass_active_stats for recognize_batch_active"""
        st = np.zeros(4, np.int64)
        self._L.ssw_grammar_active_stats(self._m, _ptr(st))
        return tuple(int(x) for x in st)

    def first_pass_active_carry(self, n_utts):
        """ssw_first_pass_active_carry: uint8 [n_utts][n_cb][n_feat][4] codewords, best first --
        what the last align_text_batch_active call with two_pass_history handed on."""
        rows = np.zeros((n_utts, self.n_cb * self.n_feat), np.uint32)
        _check(self._L.ssw_first_pass_active_carry(self._m, n_utts, _ptr(rows)),
               "ssw_first_pass_active_carry")
        return rows.view(np.uint8).reshape(n_utts, self.n_cb, self.n_feat, 4)

    # ---- alignment ----------------------------------------------------------------
    def align_batch(self, d_senscr, frame_off, phone_off, senid, tmatid, sf=None, ef=None,
                    state_init=None, stream=None):
        """Viterbi forced alignment of a batch; returns (states[n,3] int32, status[n_utts]).
        senid: [total_phones][n_emit] (n_emit = the transition matrices', 3 unless the model says
        otherwise)."""
        ne = self.tmat_n_emit
        frame_off = np.ascontiguousarray(frame_off, np.int32)
        phone_off = np.ascontiguousarray(phone_off, np.int32)
        senid = np.ascontiguousarray(senid, np.uint16).reshape(-1, ne)
        n_ph = senid.shape[0]
        tmatid = np.ascontiguousarray(tmatid, np.int16)
        sf = np.zeros(n_ph, np.int32) if sf is None else np.ascontiguousarray(sf, np.int32)
        ef = (np.full(n_ph, INT_MAX, np.int32) if ef is None
              else np.ascontiguousarray(ef, np.int32))
        states = (np.zeros((n_ph * ne, 3), np.int32) if state_init is None
                  else np.ascontiguousarray(state_init, np.int32).copy())
        n_utts = len(frame_off) - 1
        status = np.zeros(n_utts, np.int32)
        _check(self._L.ssw_align_batch(self._m, _ptr(d_senscr), n_utts, _ptr(frame_off),
                                       _ptr(phone_off), _ptr(senid), _ptr(tmatid), _ptr(sf),
                                       _ptr(ef), _ptr(states), _ptr(status),
                                       C.c_void_p(int(stream)) if stream else None),
               "ssw_align_batch")
        return states, status

    def align_batch_active(self, d_feats, frame_off, phone_off, senid, tmatid, sf=None, ef=None,
                           seed_active=None, state_init=None, d_senscr=None, stream=None,
                           scorer=None):
        """ssw_align_batch_active: scoring over the search's active senones (compallsen = no) +
        forced alignment; returns (states[n,3] int32, status[n_utts])."""
        frame_off = np.ascontiguousarray(frame_off, np.int32)
        phone_off = np.ascontiguousarray(phone_off, np.int32)
        senid = np.ascontiguousarray(senid, np.uint16).reshape(-1, 3)
        n_ph = senid.shape[0]
        tmatid = np.ascontiguousarray(tmatid, np.int16)
        sf = np.zeros(n_ph, np.int32) if sf is None else np.ascontiguousarray(sf, np.int32)
        ef = (np.full(n_ph, INT_MAX, np.int32) if ef is None
              else np.ascontiguousarray(ef, np.int32))
        states = (np.zeros((n_ph * 3, 3), np.int32) if state_init is None
                  else np.ascontiguousarray(state_init, np.int32).copy())
        n_utts = len(frame_off) - 1
        status = np.zeros(n_utts, np.int32)
        seed = None if seed_active is None else np.ascontiguousarray(seed_active, np.uint32)
        _check(self._L.ssw_align_batch_active_ex(
            self._m, self.pick_scorer(scorer), _ptr(d_feats), n_utts, _ptr(frame_off), _ptr(phone_off), _ptr(senid),
            _ptr(tmatid), _ptr(sf), _ptr(ef), _ptr(seed), _ptr(states), _ptr(status),
            _ptr(d_senscr), C.c_void_p(int(stream)) if stream else None),
            "ssw_align_batch_active")
        return states, status

    # ---- compact score rows (ssw_amd.h, "Compact score rows") -----------------------
    def compact_plan(self, frame_off, phone_off, senid, stream=None) -> "CompactPlan":
        return CompactPlan(self, frame_off, phone_off, senid, stream)

    def score_batch_compact(self, d_feats, plan, d_compact, stream=None, scorer=None,
                            share_device=False):
        """ssw_score_batch_compact: the plan's batch scored into rows that hold each
        utterance's own states only; asynchronous on `stream`."""
        _check(self._L.ssw_score_batch_compact(self._m, self.pick_scorer(scorer), _ptr(d_feats), plan._p,
                                               _ptr(d_compact),
                                               C.c_void_p(int(stream)) if stream else None,
                                               2 if share_device else 0), "ssw_score_batch_compact")

    def align_batch_compact(self, plan, d_compact, tmatid, sf=None, ef=None, state_init=None,
                            stream=None, out=None):
        """ssw_align_batch_compact; returns (states[n,3] int32, status[n_utts]).  Without
        state_init the entries are output only (SSW_ALIGN_STATE_OUT_ONLY: nothing uploaded;
        `out`, if given, is the int32 [n,3] array they are written to, whatever it held)."""
        n_ph = plan.total_phones
        tmatid = np.ascontiguousarray(tmatid, np.int16)
        assert len(tmatid) == n_ph
        sf = np.zeros(n_ph, np.int32) if sf is None else np.ascontiguousarray(sf, np.int32)
        ef = (np.full(n_ph, INT_MAX, np.int32) if ef is None
              else np.ascontiguousarray(ef, np.int32))
        if state_init is not None:
            states = np.ascontiguousarray(state_init, np.int32).copy()
        elif out is not None:
            assert out.dtype == np.int32 and out.shape == (n_ph * 3, 3) and out.flags.c_contiguous
            states = out
        else:
            states = np.empty((n_ph * 3, 3), np.int32)
        status = np.zeros(plan.n_utts, np.int32)
        _check(self._L.ssw_align_batch_compact(self._m, plan._p, _ptr(d_compact), _ptr(tmatid),
                                               _ptr(sf), _ptr(ef), _ptr(states), _ptr(status),
                                               C.c_void_p(int(stream)) if stream else None,
                                               1 if state_init is None else 0),
               "ssw_align_batch_compact")
        return states, status

    def propagate(self, child, parent, n_parent):
        child = np.ascontiguousarray(child, np.int32)
        parent = np.ascontiguousarray(parent, np.int32)
        out = np.zeros((n_parent, 3), np.int32)
        _check(self._L.ssw_alignment_propagate(_ptr(child), _ptr(parent), len(parent), _ptr(out),
                                               n_parent), "ssw_alignment_propagate")
        return out

    # ---- dynamic features ------------------------------------------------------------
    def feat_batch(self, cep, utt_off=None) -> np.ndarray:
        """Batch CMN + 1s_c_d_dd on the GPU: host MFCC [n][ncep] -> host features [n][3*ncep]."""
        cep = np.ascontiguousarray(cep, np.float32)
        n, ncep = cep.shape
        off = (np.array([0, n], np.int32) if utt_off is None
               else np.ascontiguousarray(utt_off, np.int32))
        out = np.zeros((n, 3 * ncep), np.float32)
        if n == 0:
            return out
        d_in = self.to_device(cep)
        d_out = _check(self._L.ssw_device_malloc(out.nbytes), "ssw_device_malloc")
        try:
            _check(self._L.ssw_feat_batch(self._m, d_in, n, _ptr(off), len(off) - 1, ncep, d_out,
                                          None), "ssw_feat_batch")
            _check(self._L.ssw_memcpy_d2h(_ptr(out), d_out, out.nbytes), "ssw_memcpy_d2h")
        finally:
            self._L.ssw_device_free(d_in)
            self._L.ssw_device_free(d_out)
        return out

    # ---- dynamic features of every configuration ---------------------------------------
    def feat_config(self, **overrides) -> "FeatConfig":
        """The feature stage's settings the model loaded from its feat_params.json (reference
        defaults for missing keys; `lda` unset = the model directory's feature_transform, if it
        has one), with `overrides` applied: feat, ceplen, cmn ("none", "batch" / "current",
        "live" / "prior"), cmninit (a string or numbers), varnorm, lda (a path), ldadim, svspec.
        None unsets a string setting."""
        c = FeatConfig()
        _check(self._L.ssw_model_feat_config(self._m, C.byref(c)), "ssw_model_feat_config")
        return c.update(**overrides)

    def feat(self, **overrides) -> "Feat":
        """ssw_feat_create: the model's feature configuration (with overrides, or cfg=FeatConfig)
        resolved, checked and with its tables on the device."""
        cfg = overrides.pop("cfg", None)
        if cfg is not None and overrides:
            raise SswError("feat(): give cfg or overrides, not both")
        if cfg is None and overrides:
            cfg = self.feat_config(**overrides)
        return Feat(self, cfg)

    def _own_feat(self) -> "Feat":
        if getattr(self, "_feat0", None) is None:
            self._feat0 = Feat(self, None)
        return self._feat0

    def feat_plain(self) -> bool:
        """Whether the helpers that go from audio compute this model's features with
        ssw_feat_batch: it read no feat_params.json, or its configuration is the plain one
        (1s_c_d_dd of 13 cepstra, batch CMN, no varnorm, no LDA, svspec absent or
        0-12/13-25/26-38).  Everything else goes through ssw_feat_batch_ex."""
        if getattr(self, "_feat_plain", None) is None:
            c = self.feat_config()
            if not c.from_file:
                try:                      # a feat_params.json that is there but cannot be used
                    Feat(self, None).free()   # is an error here, as it is for the front end
                except SswError as e:
                    if "feat_params.json cannot be used" in str(e):
                        raise
            self._feat_plain = (not c.from_file) or (
                c.feat == b"1s_c_d_dd" and c.ceplen in (0, 13) and c.cmn == CMN_TYPES["batch"]
                and not c.varnorm and not c.lda and c.svspec in (b"", b"0-12/13-25/26-38"))
        return self._feat_plain

    def feat_batch_ex_device(self, d_cep, n_frames, utt_off, d_out, feat=None, cmn_state=None,
                             stream=None, ncep=None):
        """ssw_feat_batch_ex on device buffers: d_cep float32 [n_frames][ceplen] -> d_out
        [n_frames][feat.out_dim].  feat None: the model's own configuration.  cmn_state: an
        SswCmnState, read and written with cmn = live."""
        feat = feat if feat is not None else self._own_feat()
        off = np.ascontiguousarray(utt_off, np.int32)
        _check(self._L.ssw_feat_batch_ex(self._m, feat._h, _ptr(d_cep), n_frames, _ptr(off),
                                         len(off) - 1, feat.ceplen if ncep is None else ncep,
                                         _ptr(d_out),
                                         None if cmn_state is None else C.byref(cmn_state),
                                         _ptr(stream)), "ssw_feat_batch_ex")

    def feat_batch_ex(self, cep, utt_off=None, feat=None, cmn_state=None) -> np.ndarray:
        """Dynamic features as the model's (or `feat`'s) configuration says, on the GPU: host
        cepstra [n][ceplen] -> host features [n][out_dim]."""
        feat = feat if feat is not None else self._own_feat()
        cep = np.ascontiguousarray(cep, np.float32)
        n, ncep = cep.shape
        off = (np.array([0, n], np.int32) if utt_off is None
               else np.ascontiguousarray(utt_off, np.int32))
        out = np.zeros((n, feat.out_dim), np.float32)
        d_in = self.to_device(cep) if n else None
        d_out = _check(self._L.ssw_device_malloc(out.nbytes), "ssw_device_malloc") if n else None
        try:
            self.feat_batch_ex_device(d_in, n, off, d_out, feat, cmn_state, ncep=ncep)
            if n:
                _check(self._L.ssw_memcpy_d2h(_ptr(out), d_out, out.nbytes), "ssw_memcpy_d2h")
        finally:
            if n:
                self._L.ssw_device_free(d_in)
                self._L.ssw_device_free(d_out)
        return out

    def _audio_feat_width(self) -> int:
        """Floats per feature row of the audio helpers: 39 for the plain configuration
        (feat_plain), else the configuration's out_dim, which must be the width of the model's
        streams together."""
        if self.feat_plain():
            return 3 * FE_NCEP
        feat = self._own_feat()
        if feat.out_dim != self.veclen_total:
            raise SswError(f"the model's feature configuration makes rows of {feat.out_dim} floats, "
                           f"but its Gaussians' streams are {self.veclen_total} wide together")
        return feat.out_dim

    def _audio_feats(self, d_cep, n_frames, fo, d_feat, stream, ncep=FE_NCEP):
        """The feature rows of the audio helpers: the plain configuration over rows of 13 cepstra
        through ssw_feat_batch, as ever; any other, and rows of another width (ssw_fe_batch_any:
        ncep, or nfilt with logspec / smoothspec), through ssw_feat_batch_ex."""
        if self.feat_plain() and ncep == FE_NCEP:
            _check(self._L.ssw_feat_batch(self._m, d_cep, n_frames, _ptr(fo), len(fo) - 1,
                                          FE_NCEP, d_feat, _ptr(stream)), "ssw_feat_batch")
        else:
            self.feat_batch_ex_device(d_cep, n_frames, fo, d_feat, None, None, stream, ncep=ncep)

    # ---- MFCC front end ----------------------------------------------------------------
    def fe_config(self, **overrides) -> SswFeConfig:
        """The front-end settings the model loaded from its feat_params.json (reference defaults
        for missing keys), with `overrides` applied, e.g. fe_config(transform="legacy")."""
        c = SswFeConfig()
        _check(self._L.ssw_model_fe_config(self._m, C.byref(c)), "ssw_model_fe_config")
        for k, v in overrides.items():
            if k not in dict(SswFeConfig._fields_):
                raise SswError(f"unknown front-end setting {k!r}")
            if k == "transform" and isinstance(v, str):
                if v not in FE_TRANSFORMS:
                    raise SswError(f"unknown transform {v!r}")
                v = FE_TRANSFORMS[v]
            setattr(c, k, int(v) if isinstance(v, bool) else v)
        return c

    def _fe_cfg(self, cfg):
        if cfg is None:
            return None                               # NULL: the model's feat_params.json
        return C.byref(cfg if isinstance(cfg, SswFeConfig) else self.fe_config(**cfg))

    def fe_batch_device(self, d_pcm, samp_off, d_cep=None, cfg=None, stream=None):
        """ssw_fe_batch: int16 PCM in HBM (torch tensor or device pointer), utterance u =
        samples samp_off[u] .. samp_off[u + 1] -> (d_cep float32 [n_frames][13] in HBM,
        frame_off int32 [n_utts + 1] on the host, as feat_batch takes them).  d_cep None: a torch
        tensor is allocated.  cfg: None (feat_params.json), a dict of overrides or an
        SswFeConfig."""
        if _pcm_kind(d_pcm, None, "fe_batch_device") == "f32":
            return self.fe_batch_f32_device(d_pcm, samp_off, None, d_cep, cfg, stream)
        off = np.ascontiguousarray(samp_off, np.int64)
        n_frames = int(fe_frame_counts(np.diff(off)).sum())
        if d_cep is None:
            import torch
            dev = d_pcm.device if hasattr(d_pcm, "device") else "cuda"
            d_cep = torch.empty((n_frames, FE_NCEP), dtype=torch.float32, device=dev)
        fo = np.zeros(len(off), np.int32)
        _check(self._L.ssw_fe_batch(self._m, self._fe_cfg(cfg), _ptr(d_pcm), _ptr(off),
                                    len(off) - 1, _ptr(d_cep), _ptr(fo), _ptr(stream)),
               "ssw_fe_batch")
        return d_cep, fo

    def fe_batch(self, pcm, samp_off=None, cfg=None):
        """The MFCC front end on the GPU, host in and host out: int16 PCM (one array, with
        samp_off for a batch, or a list of arrays) -> (cep float32 [n_frames][13], frame_off).
        float32 samples (np.float32, the reference's fe_process_float32 scale: 1.0 is 32768)
        go through ssw_fe_batch_f32 at the configuration's rate, as fe_batch_rates takes them;
        any other float type raises."""
        kind = _pcm_kind(pcm, None, "fe_batch")
        if kind == "f32":
            return self.fe_batch_rates(pcm, None, samp_off, cfg)
        pcm, off_ = _pcm_concat(pcm, kind)
        samp_off = samp_off if off_ is None else off_
        off = (np.array([0, len(pcm)], np.int64) if samp_off is None
               else np.ascontiguousarray(samp_off, np.int64))
        if len(off) < 1 or off[-1] != len(pcm):
            raise SswError("fe_batch: samp_off must end at len(pcm)")
        n_frames = int(fe_frame_counts(np.diff(off)).sum())
        cep = np.zeros((n_frames, FE_NCEP), np.float32)
        # (a model without a device gets NULL pointers: ssw_fe_batch checks the configuration,
        # then refuses the work)
        on_dev = n_frames > 0 and self.device != SSW_DEVICE_NONE
        d_pcm = self.to_device(pcm) if on_dev else None
        d_cep = self.device_malloc(cep.nbytes) if on_dev else None
        try:
            _, fo = self.fe_batch_device(d_pcm, off, d_cep if d_cep else 0, cfg)
            if on_dev:
                _check(self._L.ssw_memcpy_d2h(_ptr(cep), d_cep, cep.nbytes), "ssw_memcpy_d2h")
        finally:
            if d_pcm:
                self.device_free(d_pcm)
            if d_cep:
                self.device_free(d_cep)
        return cep, fo

    def fe_frame_counts_rates(self, n_samples, samprate=None, cfg=None) -> np.ndarray:
        """ssw_fe_frame_count_ex per utterance: samprate a number, one per utterance, or None
        for the configuration's samprate.  Raises what ssw_fe_batch_ex would refuse."""
        n = np.asarray(n_samples, np.int64).reshape(-1)
        if samprate is None:
            samprate = (cfg if isinstance(cfg, SswFeConfig) else self.fe_config(**(cfg or {}))).samprate
        sr = np.broadcast_to(np.asarray(samprate, np.float64), n.shape)
        c = self._fe_cfg(cfg)
        out = np.array([self._L.ssw_fe_frame_count_ex(self._m, c, float(r), int(k))
                        for k, r in zip(n, sr)], np.int64)
        if (out < 0).any():
            raise SswError("ssw_fe_frame_count_ex: " + _lib.last_error())
        return out

    def _fe_entry(self, kind):
        return ((self._L.ssw_fe_batch_f32, "ssw_fe_batch_f32") if kind == "f32" else
                (self._L.ssw_fe_batch_ex, "ssw_fe_batch_ex"))

    def fe_batch_rates_device(self, d_pcm, samp_off, samprate, d_cep=None, cfg=None, stream=None,
                              pcm_format=None):
        """ssw_fe_batch_ex: fe_batch_device with utterance u at samprate[u] Hz (a number for all,
        one per utterance, or None for the configuration's samprate).  A torch.float32 tensor,
        or a device pointer with pcm_format="f32", goes through ssw_fe_batch_f32."""
        fn, who = self._fe_entry(_pcm_kind(d_pcm, pcm_format, "fe_batch_rates_device"))
        off = np.ascontiguousarray(samp_off, np.int64)
        n_utts = len(off) - 1
        rates = (None if samprate is None else
                 np.ascontiguousarray(np.broadcast_to(np.asarray(samprate, np.float64), (n_utts,))))
        if d_cep is None:
            n_frames = int(self.fe_frame_counts_rates(np.diff(off), rates, cfg).sum())
            import torch
            dev = d_pcm.device if hasattr(d_pcm, "device") else "cuda"
            d_cep = torch.empty((n_frames, FE_NCEP), dtype=torch.float32, device=dev)
        fo = np.zeros(len(off), np.int32)
        _check(fn(self._m, self._fe_cfg(cfg), _ptr(d_pcm), _ptr(off), _ptr(rates), n_utts,
                  _ptr(d_cep), _ptr(fo), _ptr(stream)), who)
        return d_cep, fo

    def fe_batch_f32_device(self, d_pcm, samp_off, samprate=None, d_cep=None, cfg=None,
                            stream=None):
        """ssw_fe_batch_f32: fe_batch_rates_device for float32 samples in HBM (torch.float32
        tensor or device pointer), scaled as fe_process_float32 takes them (1.0 is 32768)."""
        return self.fe_batch_rates_device(d_pcm, samp_off, samprate, d_cep, cfg, stream,
                                          pcm_format="f32")

    def fe_batch_rates(self, pcm, samprate, samp_off=None, cfg=None):
        """The front end at each utterance's own rate, host in and host out (ssw_fe_batch_ex;
        ssw_fe_batch_f32 for np.float32 samples): PCM as fe_batch takes it, samprate a number or
        one per utterance (None: the configuration's) -> (cep float32 [n_frames][13],
        frame_off)."""
        kind = _pcm_kind(pcm, None, "fe_batch_rates")
        pcm, off_ = _pcm_concat(pcm, kind)
        samp_off = samp_off if off_ is None else off_
        off = (np.array([0, len(pcm)], np.int64) if samp_off is None
               else np.ascontiguousarray(samp_off, np.int64))
        if len(off) < 1 or off[-1] != len(pcm):
            raise SswError("fe_batch_rates: samp_off must end at len(pcm)")
        n_utts = len(off) - 1
        rates = (None if samprate is None else
                 np.ascontiguousarray(np.broadcast_to(np.asarray(samprate, np.float64), (n_utts,))))
        fn, who = self._fe_entry(kind)
        # (the entry without a device or frames checks everything, then writes frame_off)
        fo = np.zeros(len(off), np.int32)
        if self.device == SSW_DEVICE_NONE or off[-1] == 0:
            _check(fn(self._m, self._fe_cfg(cfg), None, _ptr(off), _ptr(rates), n_utts, None,
                      _ptr(fo), None), who)
        n_frames = int(fo[-1]) if fo[-1] or off[-1] == 0 else \
            int(self.fe_frame_counts_rates(np.diff(off), rates, cfg).sum())
        cep = np.zeros((n_frames, FE_NCEP), np.float32)
        if n_frames == 0:
            return cep, fo
        d_pcm = self.to_device(pcm)
        d_cep = self.device_malloc(cep.nbytes)
        try:
            _, fo = self.fe_batch_rates_device(d_pcm, off, rates, d_cep, cfg, pcm_format=kind)
            _check(self._L.ssw_memcpy_d2h(_ptr(cep), d_cep, cep.nbytes), "ssw_memcpy_d2h")
        finally:
            self.device_free(d_pcm)
            self.device_free(d_cep)
        return cep, fo

    def fe_kernel_timing(self):
        """ms per front-end kernel of the last timed fe call: (spectrum, noise, cepstrum)."""
        ms = (C.c_float * 3)()
        _check(self._L.ssw_fe_kernel_timing(self._m, ms), "ssw_fe_kernel_timing")
        return tuple(ms)

    # ---- the front end under any settings fe_init accepts ----------------------------
    def fe(self, cfg=None, warp_type=None, warp_params=None) -> "Fe":
        """ssw_fe_create: a front-end configuration resolved and checked on the host.  cfg None:
        the model's feat_params.json with the warp strings it read there; else a dict of
        overrides or an SswFeConfig, with warp_type ("inverse_linear", "affine",
        "piecewise_linear") and warp_params (e.g. "0.9 3000") beside it."""
        return Fe(self, cfg, warp_type, warp_params)

    def fe_plain(self) -> bool:
        """ssw_model_fe_plain: whether ssw_fe_batch_ex takes the model's own front-end settings.
        When not, the helpers that go from audio use ssw_fe_batch_any."""
        return bool(_check(self._L.ssw_model_fe_plain(self._m), "ssw_model_fe_plain"))

    def fe_warp(self):
        """ssw_model_fe_warp: ("warp_type", "warp_params") of the model's feat_params.json,
        ("inverse_linear", "") when it names none."""
        t, p = C.create_string_buffer(32), C.create_string_buffer(256)
        _check(self._L.ssw_model_fe_warp(self._m, t, len(t), p, len(p)), "ssw_model_fe_warp")
        return t.value.decode(), p.value.decode()

    def _own_fe(self) -> "Fe":
        if getattr(self, "_fe0", None) is None:
            self._fe0 = Fe(self)
        return self._fe0

    def fe_batch_any_device(self, d_pcm, samp_off, samprate=None, d_cep=None, fe=None,
                            stream=None, pcm_format=None):
        """ssw_fe_batch_any on device buffers: int16 or float32 samples in HBM (torch tensor, or
        a device pointer with pcm_format) -> (d_cep float32 [n_frames][fe.out_dim], frame_off).
        fe None: the model's own settings; samprate as fe_batch_rates_device takes it."""
        fe = fe if fe is not None else self._own_fe()
        kind = _pcm_kind(d_pcm, pcm_format, "fe_batch_any_device")
        off = np.ascontiguousarray(samp_off, np.int64)
        n_utts = len(off) - 1
        rates = (None if samprate is None else
                 np.ascontiguousarray(np.broadcast_to(np.asarray(samprate, np.float64), (n_utts,))))
        if d_cep is None:
            import torch
            n_frames = int(fe.frames(np.diff(off), rates).sum())
            dev = d_pcm.device if hasattr(d_pcm, "device") else "cuda"
            d_cep = torch.empty((n_frames, fe.out_dim), dtype=torch.float32, device=dev)
        fo = np.zeros(len(off), np.int32)
        _check(self._L.ssw_fe_batch_any(self._m, fe._h, _ptr(d_pcm), int(kind == "f32"), _ptr(off),
                                        _ptr(rates), n_utts, _ptr(d_cep), _ptr(fo), _ptr(stream)),
               "ssw_fe_batch_any")
        return d_cep, fo

    def fe_batch_any(self, pcm, samprate=None, fe=None, samp_off=None):
        """The front end under any settings, host in and host out: PCM as fe_batch_rates takes it
        (int16, or np.float32 where 1.0 is 32768) -> (rows float32 [n_frames][fe.out_dim],
        frame_off).  fe None: the model's own settings (Model.fe())."""
        fe = fe if fe is not None else self._own_fe()
        kind = _pcm_kind(pcm, None, "fe_batch_any")
        pcm, off_ = _pcm_concat(pcm, kind)
        samp_off = samp_off if off_ is None else off_
        off = (np.array([0, len(pcm)], np.int64) if samp_off is None
               else np.ascontiguousarray(samp_off, np.int64))
        if len(off) < 1 or off[-1] != len(pcm):
            raise SswError("fe_batch_any: samp_off must end at len(pcm)")
        n_utts = len(off) - 1
        rates = (None if samprate is None else
                 np.ascontiguousarray(np.broadcast_to(np.asarray(samprate, np.float64), (n_utts,))))
        # (the entry without a device or frames checks everything, then writes frame_off)
        fo = np.zeros(len(off), np.int32)
        if self.device == SSW_DEVICE_NONE or off[-1] == 0:
            _check(self._L.ssw_fe_batch_any(self._m, fe._h, None, int(kind == "f32"), _ptr(off),
                                            _ptr(rates), n_utts, None, _ptr(fo), None),
                   "ssw_fe_batch_any")
        n_frames = int(fo[-1]) if fo[-1] or off[-1] == 0 else int(fe.frames(np.diff(off), rates).sum())
        cep = np.zeros((n_frames, fe.out_dim), np.float32)
        if n_frames == 0:
            return cep, fo
        d_pcm = self.to_device(pcm)
        d_cep = self.device_malloc(cep.nbytes)
        try:
            _, fo = self.fe_batch_any_device(d_pcm, off, rates, d_cep, fe, pcm_format=kind)
            _check(self._L.ssw_memcpy_d2h(_ptr(cep), d_cep, cep.nbytes), "ssw_memcpy_d2h")
        finally:
            self.device_free(d_pcm)
            self.device_free(d_cep)
        return cep, fo

    # ---- device memory (no torch needed) --------------------------------------------
    def to_device(self, arr: np.ndarray) -> int:
        arr = np.ascontiguousarray(arr)
        p = _check(self._L.ssw_device_malloc(arr.nbytes), "ssw_device_malloc")
        _check(self._L.ssw_memcpy_h2d(p, _ptr(arr), arr.nbytes), "ssw_memcpy_h2d")
        return p

    def device_malloc(self, nbytes: int) -> int:
        return _check(self._L.ssw_device_malloc(int(nbytes)), "ssw_device_malloc")

    def device_free(self, p):
        self._L.ssw_device_free(p)


class Fe:
    """An ssw_fe_t: front-end settings resolved as fe_init resolves them, warp parameters
    included (Model.fe).  Host state only."""

    def __init__(self, model: Model, cfg=None, warp_type=None, warp_params=None):
        self._L = model._L
        self._model = model
        c = None if cfg is None else (cfg if isinstance(cfg, SswFeConfig) else model.fe_config(**cfg))
        self._h = self._L.ssw_fe_create(
            model._m, None if c is None else C.byref(c),
            None if warp_type is None else warp_type.encode(),
            None if warp_params is None else warp_params.encode())
        if not self._h:
            raise SswError("ssw_fe_create: " + _lib.last_error())
        self.out_dim = int(self._L.ssw_fe_out_dim(self._h))
        self.samprate = float((c if c is not None else model.fe_config()).samprate)

    def frames(self, n, rate=None) -> np.ndarray:
        """ssw_fe_frames per utterance: n samples each at rate Hz (a number, one per utterance,
        or None for the configuration's samprate)"""
        n = np.asarray(n, np.int64)
        sr = np.broadcast_to(np.asarray(self.samprate if rate is None else rate, np.float64),
                             n.shape)
        out = np.array([self._L.ssw_fe_frames(self._h, float(r), int(k))
                        for k, r in zip(n.reshape(-1), sr.reshape(-1))], np.int64).reshape(n.shape)
        if (out < 0).any():
            raise SswError("ssw_fe_frames: " + _lib.last_error())
        return out

    def free(self):
        if getattr(self, "_h", None):
            self._L.ssw_fe_free(self._h)
            self._h = None

    __del__ = free


class Feat:
    """An ssw_feat_t: a feature configuration resolved as feat_init_s3file resolves it, with its
    tables on the device (Model.feat)."""

    def __init__(self, model: Model, cfg=None):
        self._L = model._L
        self._model = model
        self._h = self._L.ssw_feat_create(model._m, None if cfg is None else C.byref(cfg))
        if not self._h:
            raise SswError("ssw_feat_create: " + _lib.last_error())
        L, h = self._L, self._h
        self.out_dim = int(L.ssw_feat_out_dim(h))
        self.raw_dim = int(L.ssw_feat_raw_dim(h))
        self.window = int(L.ssw_feat_window(h))
        self.tile_frames = int(L.ssw_feat_tile_frames(h))
        self.stream_lens = [int(L.ssw_feat_stream_len(h, i))
                            for i in range(int(L.ssw_feat_n_streams(h)))]
        self.ceplen = int((cfg if cfg is not None else model.feat_config()).ceplen) or 13

    def cmn_prior(self) -> SswCmnState:
        """ssw_feat_cmn_prior: the state of a fresh decoder (cmninit)."""
        s = SswCmnState()
        _check(self._L.ssw_feat_cmn_prior(self._h, C.byref(s)), "ssw_feat_cmn_prior")
        return s

    def free(self):
        if getattr(self, "_h", None):
            self._L.ssw_feat_free(self._h)
            self._h = None

    __del__ = free


class CompactPlan:
    """ssw_compact_plan_t: which states each utterance of a batch will be aligned against, so
    that the scorer stores their scores only (0.9 KB instead of 10 KB per frame of en-us)."""

    def __init__(self, model: Model, frame_off, phone_off, senid, stream=None):
        frame_off = np.ascontiguousarray(frame_off, np.int32)
        phone_off = np.ascontiguousarray(phone_off, np.int32)
        senid = np.ascontiguousarray(senid, np.uint16).reshape(-1, 3)
        self._L = model._L
        self.n_utts = len(frame_off) - 1
        self.total_phones = int(phone_off[-1])
        assert len(phone_off) == self.n_utts + 1 and len(senid) == self.total_phones
        self._p = self._L.ssw_compact_plan_create(model._m, self.n_utts, _ptr(frame_off),
                                                  _ptr(phone_off), _ptr(senid),
                                                  C.c_void_p(int(stream)) if stream else None)
        if not self._p:
            raise SswError("ssw_compact_plan_create: " + _lib.last_error())
        self.elems = int(self._L.ssw_compact_plan_elems(self._p))
        self.nbytes = 2 * self.elems

    def rows(self, u):
        """(offset in int16 elements, row length) of utterance u's rows in the compact buffer"""
        off, stride = C.c_longlong(0), C.c_int32(0)
        _check(self._L.ssw_compact_plan_rows(self._p, int(u), C.byref(off), C.byref(stride)),
               "ssw_compact_plan_rows")
        return int(off.value), int(stride.value)

    def free(self):
        if getattr(self, "_p", None):
            self._L.ssw_compact_plan_free(self._p)
            self._p = None

    __del__ = free


class PtmMgau:
    """`mgau_t` stand-in created by ssw_ptm_mgau_init; call through its vtable."""

    def __init__(self, model: Model):
        self._L = _lib.lib()
        self.model = model
        self._g = self._L.ssw_ptm_mgau_init(model._m)
        if not self._g:
            raise SswError("ssw_ptm_mgau_init: " + _lib.last_error())

    @property
    def name(self):
        return self._g.contents.vt.contents.name.decode()

    @property
    def frame_idx(self):
        return self._g.contents.frame_idx

    @frame_idx.setter
    def frame_idx(self, v):
        self._g.contents.frame_idx = int(v)  # acmod writes this field directly

    def reset_hist(self):
        self._L.ssw_mgau_reset_hist(self._g)

    def prescore(self, feats):
        feats = np.ascontiguousarray(feats, np.float32).reshape(-1, self.model.veclen_total)
        _check(self._L.ssw_mgau_prescore(self._g, _ptr(feats), feats.shape[0]),
               "ssw_mgau_prescore")

    def frame_eval(self, feat, frame, compallsen=True, senone_active=None):
        m = self.model
        feat = np.ascontiguousarray(feat, np.float32).reshape(-1)
        streams = (C.POINTER(C.c_float) * m.n_feat)()
        off = 0
        for f in range(m.n_feat):
            streams[f] = C.cast(feat[off:].ctypes.data, C.POINTER(C.c_float))
            off += m.veclen[f]
        out = np.zeros(m.n_sen, np.int16)
        act = None if senone_active is None else np.ascontiguousarray(senone_active, np.uint8)
        rv = self._g.contents.vt.contents.frame_eval(
            C.cast(self._g, C.c_void_p), _ptr(out), _ptr(act),
            0 if act is None else len(act), streams, int(frame), int(bool(compallsen)))
        _check(rv, "frame_eval")
        return out

    def transform(self, mllr=None):
        """the vtable's transform slot: an Mllr is applied to the model behind the scorer (0, or
        -1 when it is refused: last_error says why); without one the slot gets NULL and
        returns -1"""
        return self._g.contents.vt.contents.transform(C.cast(self._g, C.c_void_p),
                                                      None if mllr is None else mllr._t)

    def free(self):
        if getattr(self, "_g", None):
            self._g.contents.vt.contents.free(C.cast(self._g, C.c_void_p))
            self._g = None

    __del__ = free


class StateAlignSearch:
    """state_align_search_init/start/step/finish over one utterance."""

    def __init__(self, model: Model, mgau: PtmMgau | None, ssid, tmatid, start=None,
                 duration=None):
        self._L = _lib.lib()
        self.model = model
        ssid = np.ascontiguousarray(ssid, np.int32)
        tmatid = np.ascontiguousarray(tmatid, np.int32)
        n = len(ssid)
        start = None if start is None else np.ascontiguousarray(start, np.int32)
        duration = None if duration is None else np.ascontiguousarray(duration, np.int32)
        self._s = self._L.ssw_state_align_search_init(
            model._m, mgau._g if mgau is not None else None, n, _ptr(ssid), _ptr(tmatid),
            _ptr(start), _ptr(duration))
        if not self._s:
            raise SswError("ssw_state_align_search_init: " + _lib.last_error())

    def start(self):
        return _check(self._L.ssw_state_align_search_start(self._s), "start")

    def step(self, feat, frame_idx):
        feat = np.ascontiguousarray(feat, np.float32).reshape(-1)
        return _check(self._L.ssw_state_align_search_step(self._s, _ptr(feat), int(frame_idx)),
                      "step")

    def finish(self):
        return _check(self._L.ssw_state_align_search_finish(self._s), "finish")

    def _entries(self, fn):
        n = C.c_int32(0)
        p = fn(self._s, C.byref(n))
        a = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_int32)), shape=(n.value, 3))
        return a.copy()

    def states(self):
        return self._entries(self._L.ssw_state_align_search_states)

    def phones(self):
        return self._entries(self._L.ssw_state_align_search_phones)

    def free(self):
        if getattr(self, "_s", None):
            self._L.ssw_state_align_search_free(self._s)
            self._s = None

    __del__ = free


class MsMgau(PtmMgau):
    """`mgau_t` stand-in created by ssw_ms_mgau_init (the "ms" scorer)."""

    def __init__(self, model: Model):
        self._L = _lib.lib()
        self.model = model
        self._g = self._L.ssw_ms_mgau_init(model._m)
        if not self._g:
            raise SswError("ssw_ms_mgau_init: " + _lib.last_error())


class S2SemiMgau(PtmMgau):
    """`mgau_t` stand-in created by ssw_s2_semi_mgau_init (the "s2_semi" scorer of a
    single-codebook model)."""

    def __init__(self, model: Model):
        self._L = _lib.lib()
        self.model = model
        self._g = self._L.ssw_s2_semi_mgau_init(model._m)
        if not self._g:
            raise SswError("ssw_s2_semi_mgau_init: " + _lib.last_error())


class Lexicon:
    """Pronunciation dictionary + alignment_populate on the host (ssw_dict_load,
    ssw_alignment_populate): words and their windows -> the per-phone rows the aligner takes."""

    def __init__(self, model: Model, dict_path=None, filler_path=None):
        self._L = _lib.lib()
        self.model = model
        enc = lambda s: None if s is None else os.fsencode(s)
        self._d = self._L.ssw_dict_load(model._m, enc(dict_path), enc(filler_path))
        if not self._d:
            raise SswError("ssw_dict_load: " + _lib.last_error())

    def __len__(self):
        return int(self._L.ssw_dict_size(self._d))

    def pron(self, word: str):
        buf = np.zeros(256, np.int32)
        n = self._L.ssw_dict_pron(self._d, word.encode(), _ptr(buf), 256)
        if n < 0:
            raise KeyError(word)
        return [self._L.ssw_ciphone_name(self.model._m, int(c)).decode() for c in buf[:n]]

    def phone_id_nearest(self, b, l, r, pos):
        return int(self._L.ssw_phone_id_nearest(self.model._m, int(b), int(l), int(r), int(pos)))

    def populate(self, words, start=None, duration=None, max_phones=21845):
        """Returns dict(ssid, tmatid, cipid, parent, start, duration) of int32 arrays."""
        n = len(words)
        arr = (C.c_char_p * n)(*[w.encode() for w in words])
        st = None if start is None else np.ascontiguousarray(start, np.int32)
        du = None if duration is None else np.ascontiguousarray(duration, np.int32)
        out = {k: np.zeros(max_phones, np.int32)
               for k in ("ssid", "tmatid", "cipid", "parent", "start", "duration")}
        k = self._L.ssw_alignment_populate(self.model._m, self._d, n, arr, _ptr(st), _ptr(du),
                                           max_phones, _ptr(out["ssid"]), _ptr(out["tmatid"]),
                                           _ptr(out["cipid"]), _ptr(out["parent"]),
                                           _ptr(out["start"]), _ptr(out["duration"]))
        _check(k, "ssw_alignment_populate")
        return {key: v[:k].copy() for key, v in out.items()}

    def alignment_json(self, hyp, words, word_al, cipid, parent, phone_al, n_frames,
                       state_senid=None, state_al=None, hyp_logprob=0, utt_start=0.0, frate=100):
        """decoder_result_json at align_level 1 (or 2 with the state level): the reference's
        one-line JSON for an alignment.  *_al: int32 [n][3] (start, duration, score)."""
        n = len(words)
        arr = (C.c_char_p * n)(*[w.encode() for w in words])
        wa = np.ascontiguousarray(word_al, np.int32).reshape(-1, 3)
        pa = np.ascontiguousarray(phone_al, np.int32).reshape(-1, 3)
        ci = np.ascontiguousarray(cipid, np.int32)
        par = np.ascontiguousarray(parent, np.int32)
        sid = None if state_senid is None else np.ascontiguousarray(state_senid, np.uint16)
        sa = None if state_al is None else np.ascontiguousarray(state_al, np.int32).reshape(-1, 3)
        args = (self.model._m, hyp.encode(), int(hyp_logprob), float(utt_start), int(frate),
                int(n_frames), n, arr, _ptr(wa), len(ci), _ptr(ci), _ptr(par), _ptr(pa), _ptr(sid),
                _ptr(sa))
        need = self._L.ssw_alignment_json(*args, None, 0)
        _check(need, "ssw_alignment_json")
        buf = C.create_string_buffer(need + 1)
        _check(self._L.ssw_alignment_json(*args, buf, need + 1), "ssw_alignment_json")
        return buf.value.decode()

    def word(self, wid: int):
        w = self._L.ssw_dict_word(self._d, int(wid))
        return None if w is None else w.decode()

    def word_id(self, word: str) -> int:
        return int(self._L.ssw_dict_word_id(self._d, word.encode()))

    def is_filler(self, wid: int) -> bool:
        """dict_filler_word: from the filler dictionary, <s> and </s> excepted."""
        return bool(self._L.ssw_dict_is_filler(self._d, int(wid)))

    def add_word(self, word: str, phones: str) -> int:
        """decoder_add_word (ssw_dict_add_word): a word and its CI phone names, separated by
        white space, appended to the loaded dictionary; "w(2)" adds an alternate of w.  Returns
        the new word id.  KeyError for a word that exists, as the reference's binding raises;
        SswError for any other refusal, the dictionary unchanged.  Graphs, plans and grammars
        built before the add are snapshots and do not know the word."""
        if self.word_id(word) >= 0:
            raise KeyError(word)
        return int(_check(self._L.ssw_dict_add_word(self._d, self.model._m, word.encode(),
                                                    phones.encode()), "ssw_dict_add_word"))

    def lookup_word(self, word: str):
        """decoder_lookup_word: the word's phone names separated by one space, None when the
        dictionary does not have it."""
        w = word.encode()
        need = self._L.ssw_dict_lookup_word(self._d, self.model._m, w, None, 0)
        if need < 0:
            return None
        buf = C.create_string_buffer(need + 1)
        self._L.ssw_dict_lookup_word(self._d, self.model._m, w, buf, need + 1)
        return buf.value.decode()

    def first_pass_config(self, **kw) -> FirstPassConfig:
        cfg = FirstPassConfig()
        self._L.ssw_first_pass_config_defaults(C.byref(cfg))
        for k, v in kw.items():
            setattr(cfg, k, v)
        return cfg

    def first_pass_graph(self, words, cfg=None, max_nodes=1 << 16):
        """The phone-tree HMMs the first pass searches for one text (host only): a structured
        array (FP_NODE_DTYPE) and the three beams."""
        arr = (C.c_char_p * len(words))(*[w.encode() for w in words])
        nodes = np.zeros(max_nodes, FP_NODE_DTYPE)
        beams = np.zeros(3, np.int32)
        n = self._L.ssw_first_pass_graph(self.model._m, self._d,
                                         None if cfg is None else C.byref(cfg), len(words), arr,
                                         max_nodes, _ptr(nodes), _ptr(beams))
        _check(n, "ssw_first_pass_graph")
        return nodes[:n].copy(), beams

    def grammar_graph(self, fsg, cfg=None, max_nodes=1 << 16):
        """The phone-tree HMMs the grammar search walks for one Fsg (host only), as
        first_pass_graph gives them for a text."""
        nodes = np.zeros(max_nodes, FP_NODE_DTYPE)
        beams = np.zeros(3, np.int32)
        n = self._L.ssw_grammar_graph(self.model._m, self._d,
                                      None if cfg is None else C.byref(cfg), fsg._f, max_nodes,
                                      _ptr(nodes), _ptr(beams))
        _check(n, "ssw_grammar_graph")
        return nodes[:n].copy(), beams

    def grammar_plan(self, fsgs, cfg=None, max_hmms=None, active=False) -> "GrammarPlan":
        """ssw_grammar_prepare: decoder_set_fsg for a list of Fsg (or one); the graphs are built
        once on the host and cached on the device while the plan is searched.  max_hmms (up to
        30000): ssw_grammar_prepare_large, grammars beyond the 4096 phone-tree HMMs one workgroup
        holds; a plan with such a grammar is searched from an HBM workspace, all of it.
        active=True (needs max_hmms): ssw_grammar_prepare_large_active, the same plan, which
        recognize_batch_active takes as well (the reference's default compallsen = no)."""
        if active and max_hmms is None:
            raise ValueError("grammar_plan(active=True) needs max_hmms: the flag is for plans of "
                             "grammars beyond one workgroup (a plan made without max_hmms is "
                             "taken by recognize_batch_active as it is)")
        return GrammarPlan(self, fsgs, cfg, max_hmms, active)

    def first_pass(self, d_senscr, utt_off, texts, cfg=None, max_seg=None, stream=None):
        """ssw_first_pass_batch: device senone scores of a batch + one word list per utterance
        -> per utterance a list of (word, start, duration, score), or None when the grammar's
        final state is not reached."""
        n_seg, seg = self.first_pass_raw(d_senscr, utt_off, texts, cfg, max_seg, stream)
        out = []
        for u in range(len(n_seg)):
            if n_seg[u] <= -2:
                raise SswError(f"first_pass: utterance {u} needs max_seg >= {-n_seg[u] - 2}")
            if n_seg[u] < 0:
                out.append(None)
            else:
                out.append([(self.word(int(s["wid"])), int(s["start"]), int(s["duration"]),
                             int(s["score"])) for s in seg[u, :n_seg[u]]])
        return out

    def first_pass_raw(self, d_senscr, utt_off, texts, cfg=None, max_seg=None, stream=None):
        """The C call alone: (n_seg int32 [n_utts], seg WORD_SEG_DTYPE [n_utts][max_seg])."""
        off = np.ascontiguousarray(utt_off, np.int32)
        n_utts = len(off) - 1
        assert len(texts) == n_utts
        word_off = np.zeros(n_utts + 1, np.int32)
        word_off[1:] = np.cumsum([len(t) for t in texts])
        flat = [w.encode() for t in texts for w in t]
        arr = (C.c_char_p * max(1, len(flat)))(*flat)
        if max_seg is None:
            max_seg = 4 * max(len(t) for t in texts) + 8
        n_seg = np.zeros(n_utts, np.int32)
        seg = np.zeros((n_utts, max_seg), WORD_SEG_DTYPE)
        _check(self._L.ssw_first_pass_batch(self.model._m, self._d,
                                            None if cfg is None else C.byref(cfg),
                                            _ptr(d_senscr), int(off[-1]), _ptr(off), n_utts,
                                            _ptr(word_off), arr, max_seg, _ptr(n_seg), _ptr(seg),
                                            _ptr(stream)), "ssw_first_pass_batch")
        return n_seg, seg

    def first_pass_active(self, d_feats, utt_off, texts, cfg=None, max_seg=None, stream=None,
                          scorer=None, d_senscr=None, want_seed=False):
        """ssw_first_pass_batch_active: the first pass in the reference's DEFAULT configuration
        (compallsen = no) for a batch, from feature rows in HBM.  Returns (segmentations as
        first_pass does, rounds int32 [n_utts]) and, with want_seed, the uint32
        [n_utts][(n_sen + 31) // 32] set acmod holds after each utterance's last frame; d_senscr
        (device int16 [n_frames][n_sen]) receives the rows as acmod's buffer would hold them."""
        n_seg, seg, rounds, seed = self.first_pass_active_raw(d_feats, utt_off, texts, cfg, max_seg,
                                                              stream, scorer, d_senscr, want_seed)
        out = []
        for u in range(len(n_seg)):
            if n_seg[u] <= -2:
                raise SswError(f"first_pass_active: utterance {u} needs max_seg >= {-n_seg[u] - 2}")
            if n_seg[u] < 0:
                out.append(None)
            else:
                out.append([(self.word(int(s["wid"])), int(s["start"]), int(s["duration"]),
                             int(s["score"])) for s in seg[u, :n_seg[u]]])
        return (out, rounds, seed) if want_seed else (out, rounds)

    def first_pass_active_raw(self, d_feats, utt_off, texts, cfg=None, max_seg=None, stream=None,
                              scorer=None, d_senscr=None, want_seed=False):
        """The C call alone: (n_seg, seg WORD_SEG_DTYPE [n_utts][max_seg], rounds, seed or None);
        texts: list of word lists, or a Texts."""
        off = np.ascontiguousarray(utt_off, np.int32)
        n_utts = len(off) - 1
        tx = texts if isinstance(texts, Texts) else Texts(texts)
        assert tx.n_utts == n_utts
        if max_seg is None:
            max_seg = 4 * tx.max_words + 8
        n_seg = np.zeros(n_utts, np.int32)
        seg = np.zeros((n_utts, max_seg), WORD_SEG_DTYPE)
        rounds = np.zeros(n_utts, np.int32)
        seed = np.zeros((n_utts, (self.model.n_sen + 31) // 32), np.uint32) if want_seed else None
        _check(self._L.ssw_first_pass_batch_active(
            self.model._m, self._d, None if cfg is None else C.byref(cfg),
            self.model.pick_scorer(scorer), _ptr(d_feats), int(off[-1]), _ptr(off), n_utts, _ptr(tx.word_off), tx.arr, max_seg,
            _ptr(n_seg), _ptr(seg), _ptr(seed), _ptr(d_senscr), _ptr(rounds), _ptr(stream)),
            "ssw_first_pass_batch_active")
        return n_seg, seg, rounds, seed

    def free(self):
        if getattr(self, "_d", None):
            self._L.ssw_dict_free(self._d)
            self._d = None

    __del__ = free


def _view(ptr, n, dtype, cols=None):
    if n <= 0 or not ptr:
        return np.zeros((0, cols) if cols else 0, dtype)
    count = n * (cols or 1)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr.value)
    arr = np.frombuffer(buf, dtype=dtype, count=count).copy()
    return arr.reshape(n, cols) if cols else arr


class AlignmentSet:
    """ssw_alignment_set_t: the alignment_t-shaped result of ssw_forced_align_batch."""

    def __init__(self, lib, handle, lex):
        self._L, self._a, self._lex = lib, handle, lex

    def status(self, u):
        return int(self._L.ssw_alignment_set_status(self._a, u))

    def message(self, u):
        """Why utterance u's text was rejected (status 3), else ''."""
        return self._L.ssw_alignment_set_message(self._a, u).decode()

    def utterance(self, u):
        """None unless status 0; else dict(words, word_al, cipid, parent, phone_al, senid,
        state_al) with *_al int32 [n][3] = (start, duration, score)."""
        if self.status(u) != 0:
            return None
        p1, p2, p3 = C.c_void_p(), C.c_void_p(), C.c_void_p()
        n = self._L.ssw_alignment_set_words(self._a, u, C.byref(p1), C.byref(p2))
        wid = _view(p1, n, np.int32)
        word_al = _view(p2, n, np.int32, 3)
        n = self._L.ssw_alignment_set_phones(self._a, u, C.byref(p1), C.byref(p2), C.byref(p3))
        cipid, parent, phone_al = _view(p1, n, np.int32), _view(p2, n, np.int32), _view(p3, n, np.int32, 3)
        n = self._L.ssw_alignment_set_states(self._a, u, C.byref(p1), C.byref(p2))
        senid, state_al = _view(p1, n, np.uint16), _view(p2, n, np.int32, 3)
        return {"wid": wid, "words": [self._lex.word(int(w)) for w in wid], "word_al": word_al,
                "cipid": cipid, "parent": parent, "phone_al": phone_al,
                "senid": senid.reshape(-1, 3), "state_al": state_al}

    def json(self, u, align_level=1, utt_start=0.0, frate=100):
        """ssw_alignment_set_json: the reference's one-line JSON for utterance u."""
        need = self._L.ssw_alignment_set_json(self._a, u, float(utt_start), frate, align_level,
                                              None, 0)
        _check(need, "ssw_alignment_set_json")
        buf = C.create_string_buffer(need + 1)
        _check(self._L.ssw_alignment_set_json(self._a, u, float(utt_start), frate, align_level,
                                              buf, need + 1), "ssw_alignment_set_json")
        return buf.value.decode()

    def free(self):
        if self._a:
            self._L.ssw_alignment_set_free(self._a)
            self._a = None

    __del__ = free


def forced_align_batch(model: Model, lex: Lexicon, d_senscr, utt_off, texts, cfg=None,
                       stream=None) -> AlignmentSet:
    """ssw_forced_align_batch: decoder_alignment (src/decoder.c:737-798) for a batch of
    utterances whose senone scores are in HBM -- first pass, populate with its word windows,
    constrained state alignment, propagate -- in one C call."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    word_off = np.zeros(n_utts + 1, np.int32)
    word_off[1:] = np.cumsum([len(t) for t in texts])
    flat = [w.encode() for t in texts for w in t]
    arr = (C.c_char_p * max(1, len(flat)))(*flat)
    L = _lib.lib()
    h = L.ssw_forced_align_batch(model._m, lex._d, None if cfg is None else C.byref(cfg),
                                 _ptr(d_senscr), int(off[-1]), _ptr(off), n_utts, _ptr(word_off),
                                 arr, _ptr(stream))
    if not h:
        raise SswError("ssw_forced_align_batch: " + _lib.last_error())
    return AlignmentSet(L, h, lex)


class FirstPassPlan:
    """ssw_first_pass_plan_t: the graphs of a batch of texts, built on the host without touching
    the device (ctypes releases the GIL: prepare the next batch on another thread while the GPU
    works on this one)."""

    def __init__(self, model: Model, lex: Lexicon, texts, cfg=None):
        self._L = _lib.lib()
        n_utts = len(texts)
        word_off = np.zeros(n_utts + 1, np.int32)
        word_off[1:] = np.cumsum([len(t) for t in texts])
        flat = [w.encode() for t in texts for w in t]
        arr = (C.c_char_p * max(1, len(flat)))(*flat)
        self.n_utts = n_utts
        self._p = self._L.ssw_first_pass_prepare(model._m, lex._d,
                                                 None if cfg is None else C.byref(cfg), n_utts,
                                                 _ptr(word_off), arr)
        if not self._p:
            raise SswError("ssw_first_pass_prepare: " + _lib.last_error())

    def free(self):
        if getattr(self, "_p", None):
            self._L.ssw_first_pass_plan_free(self._p)
            self._p = None

    __del__ = free


def forced_align_planned(model: Model, lex: Lexicon, plan: FirstPassPlan, d_senscr, utt_off,
                         stream=None) -> AlignmentSet:
    """ssw_forced_align_planned: forced_align_batch with the graphs prepared beforehand."""
    off = np.ascontiguousarray(utt_off, np.int32)
    assert len(off) - 1 == plan.n_utts
    L = _lib.lib()
    h = L.ssw_forced_align_planned(model._m, lex._d, plan._p, _ptr(d_senscr), int(off[-1]),
                                   _ptr(off), _ptr(stream))
    if not h:
        raise SswError("ssw_forced_align_planned: " + _lib.last_error())
    return AlignmentSet(L, h, lex)


class Texts:
    """The texts of a batch as the C calls take them (word_off + char **), marshalled once:
    turning a few thousand Python strings into a ctypes array costs about a millisecond, which a
    caller that aligns the same texts again (or a C host) does not pay."""

    def __init__(self, texts):
        self.n_utts = len(texts)
        self.word_off = np.zeros(self.n_utts + 1, np.int32)
        self.word_off[1:] = np.cumsum([len(t) for t in texts])
        self._flat = [w.encode() for t in texts for w in t]
        self.arr = (C.c_char_p * max(1, len(self._flat)))(*self._flat)
        self.max_words = max((len(t) for t in texts), default=0)

    def __len__(self):
        return self.n_utts


def align_text_batch(model: Model, lex: Lexicon, d_feats, utt_off, texts, cfg=None,
                     scorer=None, stream=None) -> AlignmentSet:
    """ssw_align_text_batch: feature rows in HBM + texts (list of word lists, or a Texts) ->
    alignments (scoring, first pass, populate, constrained state alignment, propagate) in one C
    call."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    tx = texts if isinstance(texts, Texts) else Texts(texts)
    assert tx.n_utts == n_utts
    L = _lib.lib()
    h = L.ssw_align_text_batch(model._m, lex._d, None if cfg is None else C.byref(cfg),
                               model.pick_scorer(scorer),
                               _ptr(d_feats), int(off[-1]), _ptr(off), n_utts, _ptr(tx.word_off),
                               tx.arr, _ptr(stream))
    if not h:
        raise SswError("ssw_align_text_batch: " + _lib.last_error())
    return AlignmentSet(L, h, lex)


def align_text_batch_active(model: Model, lex: Lexicon, d_feats, utt_off, texts, cfg=None,
                            scorer=None, stream=None) -> AlignmentSet:
    """ssw_align_text_batch_active: align_text_batch in the reference's DEFAULT configuration
    (compallsen = no): both passes score what their searches hold active."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    tx = texts if isinstance(texts, Texts) else Texts(texts)
    assert tx.n_utts == n_utts
    L = _lib.lib()
    h = L.ssw_align_text_batch_active(model._m, lex._d, None if cfg is None else C.byref(cfg),
                                      model.pick_scorer(scorer), _ptr(d_feats), int(off[-1]),
                                      _ptr(off), n_utts, _ptr(tx.word_off), tx.arr, _ptr(stream))
    if not h:
        raise SswError("ssw_align_text_batch_active: " + _lib.last_error())
    return AlignmentSet(L, h, lex)


class _AudioIn:
    """The audio helpers' way in: the batch's samples in HBM and its cepstra.  int16 audio goes
    as ever (ssw_fe_batch when samprate is None, else ssw_fe_batch_ex); float32 audio (np.float32
    array, torch.float32 device tensor, or a device pointer with pcm_format="f32") through
    ssw_fe_batch_f32, at the configuration's rate when samprate is None."""

    def __init__(self, model: Model, pcm, samp_off, samprate, fe_cfg, pcm_format, who):
        self.model = model
        self.kind = _pcm_kind(pcm, pcm_format, who)
        self.off = np.ascontiguousarray(samp_off, np.int64)
        self.samprate = samprate
        self.fe_cfg = fe_cfg
        n = np.diff(self.off)
        # ssw_fe_batch_any in exactly two cases: the caller's Fe, or no fe_cfg and settings of
        # the model's own that the older entry points refuse
        self.fe = fe_cfg if isinstance(fe_cfg, Fe) else (
            model._own_fe() if fe_cfg is None and not model.fe_plain() else None)
        self.ncep = FE_NCEP if self.fe is None else self.fe.out_dim
        if self.fe is not None:
            self.n_frames = int(self.fe.frames(n, samprate).sum())
        else:
            self.n_frames = int(fe_frame_counts(n).sum() if samprate is None and self.kind == "i16"
                                else model.fe_frame_counts_rates(n, samprate, fe_cfg).sum())
        self.on_device = _is_device_tensor(pcm) or isinstance(pcm, (int, C.c_void_p))
        self.d_pcm = pcm if self.on_device else (
            model.to_device(np.ascontiguousarray(pcm, _PCM_DTYPE[self.kind]))
            if self.off[-1] > 0 else None)

    def cepstra(self, d_cep, stream):
        m = self.model
        if self.fe is not None:
            return m.fe_batch_any_device(self.d_pcm, self.off, self.samprate, d_cep, self.fe,
                                         stream, pcm_format=self.kind)[1]
        if self.kind == "f32":
            return m.fe_batch_f32_device(self.d_pcm, self.off, self.samprate, d_cep, self.fe_cfg,
                                         stream)[1]
        if self.samprate is None:
            return m.fe_batch_device(self.d_pcm, self.off, d_cep, self.fe_cfg, stream)[1]
        return m.fe_batch_rates_device(self.d_pcm, self.off, self.samprate, d_cep, self.fe_cfg,
                                       stream)[1]

    def free(self):
        if self.d_pcm is not None and not self.on_device:
            self.model.device_free(self.d_pcm)
        self.d_pcm = None


def align_audio_batch(model: Model, lex: Lexicon, pcm, samp_off, texts, cfg=None, active=False,
                      fe_cfg=None, scorer=None, stream=None, samprate=None,
                      pcm_format=None) -> AlignmentSet:
    """Audio and text in, alignments out: what decoder_process_int16 over each utterance and
    decoder_alignment give (src/decoder.c:737-798), for a batch.  int16 PCM (host array or
    device tensor; utterance u = samples samp_off[u] .. samp_off[u + 1]) -> ssw_fe_batch ->
    ssw_feat_batch (ssw_feat_batch_ex when the model's feat_params.json asks for anything but
    the plain features, Model.feat_plain) -> ssw_align_text_batch, or ssw_align_text_batch_active when active=True (the
    reference's default compallsen = no).  cfg: FirstPassConfig; fe_cfg: front-end settings
    (None = the model's feat_params.json).  samprate None: 16 kHz audio through ssw_fe_batch;
    a number, or one per utterance: the cepstra at that rate through ssw_fe_batch_ex, as the
    reference computes them at the rate the audio has.  float32 audio (np.float32 array,
    torch.float32 device tensor, or a device pointer with pcm_format="f32"; 1.0 is 32768) is
    what decoder_process_float32 takes (src/decoder.c:960-1000) and goes through
    ssw_fe_batch_f32; arrays and tensors of any other float type raise.  The cepstra come
    from ssw_fe_batch_any instead in two cases: fe_cfg is an Fe (Model.fe), or fe_cfg is None and
    the model's own settings are ones only that entry takes (Model.fe_plain is False: remove_dc,
    round_filters = no, warping, ...); their rows, fe.out_dim wide, go on to the feature stage."""
    width = model._audio_feat_width()
    audio = _AudioIn(model, pcm, samp_off, samprate, fe_cfg, pcm_format, "align_audio_batch")
    n_frames = audio.n_frames
    d_cep = model.device_malloc(n_frames * audio.ncep * 4) if n_frames else None
    d_feat = model.device_malloc(n_frames * width * 4) if n_frames else None
    try:
        fo = audio.cepstra(d_cep if d_cep else 0, stream)
        if n_frames:
            model._audio_feats(d_cep, n_frames, fo, d_feat, stream, audio.ncep)
        fn = align_text_batch_active if active else align_text_batch
        return fn(model, lex, d_feat if d_feat else 0, fo, texts, cfg=cfg, scorer=scorer,
                  stream=stream)
    finally:
        audio.free()
        for p in (d_cep, d_feat):
            if p:
                model.device_free(p)


def forced_alignment(model: Model, lex: Lexicon, d_senscr, utt_off, texts, cfg=None, stream=None):
    """forced_align_batch, unpacked: one dict per utterance, None where it could not be aligned."""
    s = forced_align_batch(model, lex, d_senscr, utt_off, texts, cfg=cfg, stream=stream)
    out = [s.utterance(u) for u in range(len(texts))]
    s.free()
    return out


FSG_SEG_DTYPE = np.dtype([("wid", "<i4"), ("sf", "<i4"), ("ef", "<i4"), ("ascr", "<i4"),
                          ("lscr", "<i4")])


class Fsg:
    """ssw_fsg_t: a word finite-state grammar (fsg_model_t), from a transition list or a .fsg
    file.  lex=None skips the dictionary check until the grammar is planned."""

    def __init__(self, handle):
        self._L = _lib.lib()
        self._f = handle

    @classmethod
    def create(cls, model: Model, lex, name, start, final, transitions, n_states=None):
        """transitions: (from, to, prob[, word]) tuples; without a word (or with None / "") a
        null transition.  n_states None: the largest state number + 1, as create_fsg counts."""
        tr = [(t[0], t[1], t[2], t[3] if len(t) > 3 and t[3] else None) for t in transitions]
        if n_states is None:
            n_states = max([start, final] + [max(t[0], t[1]) for t in tr]) + 1
        n = len(tr)
        fr = np.array([t[0] for t in tr], np.int32)
        to = np.array([t[1] for t in tr], np.int32)
        pr = np.array([t[2] for t in tr], np.float32)
        words = (C.c_char_p * max(1, n))(*[None if t[3] is None else t[3].encode() for t in tr])
        L = _lib.lib()
        h = L.ssw_fsg_create(model._m, None if lex is None else lex._d, name.encode(),
                             int(n_states), int(start), int(final), n, _ptr(fr), _ptr(to),
                             _ptr(pr), words)
        if not h:
            raise SswError("ssw_fsg_create: " + _lib.last_error())
        return cls(h)

    @classmethod
    def read(cls, model: Model, lex, path):
        L = _lib.lib()
        h = L.ssw_fsg_read(model._m, None if lex is None else lex._d, os.fsencode(path))
        if not h:
            raise SswError("ssw_fsg_read: " + _lib.last_error())
        return cls(h)

    @classmethod
    def from_jsgf(cls, model: Model, lex, text=None, path=None, toprule=None):
        """decoder_set_jsgf_string (text) / decoder_set_jsgf_file (path) up to decoder_set_fsg:
        toprule "grammar.rule", or the first public rule in the reference's order."""
        if (text is None) == (path is None):
            raise ValueError("Fsg.from_jsgf takes either text or path")
        L = _lib.lib()
        top = None if toprule is None else toprule.encode()
        d = None if lex is None else lex._d
        if text is not None:
            who = "ssw_fsg_from_jsgf_string"
            h = L.ssw_fsg_from_jsgf_string(model._m, d, text.encode() if isinstance(text, str) else text, top)
        else:
            who = "ssw_fsg_from_jsgf_file"
            h = L.ssw_fsg_from_jsgf_file(model._m, d, os.fsencode(path), top)
        if not h:
            raise SswError(who + ": " + _lib.last_error())
        return cls(h)

    @property
    def name(self):
        return self._L.ssw_fsg_name(self._f).decode()

    @property
    def n_states(self):
        return int(self._L.ssw_fsg_n_states(self._f))

    def write(self, lex=None, cfg=None, searched=False) -> str:
        """fsg_model_write: the grammar as read (null transitions closed) or, with
        searched=True, as the search sees it (silences and alternates added)."""
        args = (self._f, None if lex is None else lex._d, None if cfg is None else C.byref(cfg),
                1 if searched else 0)
        need = self._L.ssw_fsg_write(*args, None, 0)
        _check(need, "ssw_fsg_write")
        buf = C.create_string_buffer(need + 1)
        _check(self._L.ssw_fsg_write(*args, buf, need + 1), "ssw_fsg_write")
        return buf.value.decode()

    def free(self):
        if getattr(self, "_f", None):
            self._L.ssw_fsg_free(self._f)
            self._f = None

    __del__ = free


class Jsgf:
    """ssw_jsgf_t: a parsed JSGF grammar (jsgf_t).  Rule indices are positions in rules(), the
    order the reference's rule table is walked in."""

    def __init__(self, handle):
        self._L = _lib.lib()
        self._j = handle

    @classmethod
    def parse_string(cls, text):
        h = _lib.lib().ssw_jsgf_parse_string(text.encode() if isinstance(text, str) else text)
        if not h:
            raise SswError("ssw_jsgf_parse_string: " + _lib.last_error())
        return cls(h)

    @classmethod
    def parse_file(cls, path):
        h = _lib.lib().ssw_jsgf_parse_file(os.fsencode(path))
        if not h:
            raise SswError("ssw_jsgf_parse_file: " + _lib.last_error())
        return cls(h)

    @property
    def name(self):
        return self._L.ssw_jsgf_name(self._j).decode()

    def rules(self):
        """[(name, is_public)] in jsgf_rule_iter order"""
        return [(self._L.ssw_jsgf_rule_name(self._j, i).decode(),
                 bool(self._L.ssw_jsgf_rule_public(self._j, i)))
                for i in range(self._L.ssw_jsgf_n_rules(self._j))]

    def public_rule(self):
        """jsgf_get_public_rule: index of the first public rule, or None"""
        i = self._L.ssw_jsgf_public_rule(self._j)
        return None if i < 0 else int(i)

    def find_rule(self, name):
        """jsgf_get_rule("grammar.rule"): index, or None"""
        i = self._L.ssw_jsgf_find_rule(self._j, name.encode())
        return None if i < 0 else int(i)

    def fsg(self, model: Model, lex, rule=None) -> Fsg:
        """jsgf_build_fsg of rule (an index, a "grammar.rule" name, or None: the first public
        rule).  As in the reference, every build renormalises the grammar's weights in place."""
        if rule is None:
            i = self.public_rule()
            if i is None:
                raise SswError("ssw_jsgf_public_rule: No public rules found in input string")
        elif isinstance(rule, str):
            i = self.find_rule(rule)
            if i is None:
                raise SswError("ssw_jsgf_find_rule: Start rule %s not found" % rule)
        else:
            i = int(rule)
        h = self._L.ssw_jsgf_build_fsg(model._m, None if lex is None else lex._d, self._j, i)
        if not h:
            raise SswError("ssw_jsgf_build_fsg: " + _lib.last_error())
        return Fsg(h)

    def free(self):
        if getattr(self, "_j", None):
            self._L.ssw_jsgf_free(self._j)
            self._j = None

    __del__ = free


class GrammarPlan:
    """ssw_grammar_plan_t: the phone-tree graphs of one or more grammars."""

    def __init__(self, lex: Lexicon, fsgs, cfg=None, max_hmms=None, active=False):
        self._L = _lib.lib()
        fsgs = [fsgs] if isinstance(fsgs, Fsg) else list(fsgs)
        self.n_fsgs = len(fsgs)
        arr = (C.c_void_p * max(1, len(fsgs)))(*[f._f for f in fsgs])
        pcfg = None if cfg is None else C.byref(cfg)
        if max_hmms is None:
            who = "ssw_grammar_prepare"
            self._p = self._L.ssw_grammar_prepare(lex.model._m, lex._d, pcfg, len(fsgs), arr)
        else:
            who = "ssw_grammar_prepare_large_active" if active else "ssw_grammar_prepare_large"
            self._p = getattr(self._L, who)(lex.model._m, lex._d, pcfg, len(fsgs), arr,
                                            int(max_hmms))
        if not self._p:
            raise SswError(who + ": " + _lib.last_error())
        # ssw_grammar_plan_active: recognize_batch_active takes the plan even where a grammar is
        # beyond one workgroup
        self.active = self._L.ssw_grammar_plan_active(self._p) == 1

    def hmms(self, fsg=0) -> int:
        return int(self._L.ssw_grammar_plan_hmms(self._p, fsg))

    def history_groups(self, utt_off, fsg_of_utt=None) -> int:
        """ssw_grammar_history_groups: the launches a search of these utterances takes"""
        off = np.ascontiguousarray(utt_off, np.int32)
        g = _fsg_of_utt(fsg_of_utt, len(off) - 1)
        n = self._L.ssw_grammar_history_groups(self._p, _ptr(g), _ptr(off), len(off) - 1)
        _check(n, "ssw_grammar_history_groups")
        return int(n)

    def free(self):
        if getattr(self, "_p", None):
            self._L.ssw_grammar_plan_free(self._p)
            self._p = None

    __del__ = free


class RecognitionSet:
    """ssw_recognition_set_t: per utterance status / message / hyp / score / segments / json."""

    def __init__(self, lib, handle, lex, n_utts):
        self._L, self._r, self._lex, self.n_utts = lib, handle, lex, n_utts

    def __len__(self):
        return self.n_utts

    def status(self, u):
        return int(self._L.ssw_recognition_set_status(self._r, u))

    def message(self, u):
        return self._L.ssw_recognition_set_message(self._r, u).decode()

    def hyp(self, u):
        """decoder_hyp's text, or None"""
        need = self._L.ssw_recognition_set_hyp(self._r, u, None, 0)
        if need < 0:
            return None
        buf = C.create_string_buffer(need + 1)
        self._L.ssw_recognition_set_hyp(self._r, u, buf, need + 1)
        return buf.value.decode()

    def score(self, u):
        v = C.c_int32()
        return int(v.value) if self._L.ssw_recognition_set_score(self._r, u, C.byref(v)) == 0 else None

    def segments_raw(self, u):
        p = C.c_void_p()
        n = self._L.ssw_recognition_set_segments(self._r, u, C.byref(p))
        return _view(p, n, FSG_SEG_DTYPE)

    def segments(self, u):
        """[(word or "(NULL)", sf, ef, ascr, lscr)] of the best path"""
        return [("(NULL)" if s["wid"] < 0 else self._lex.word(int(s["wid"])), int(s["sf"]),
                 int(s["ef"]), int(s["ascr"]), int(s["lscr"])) for s in self.segments_raw(u)]

    def json(self, u, utt_start=0.0, frate=100):
        """the line decoder_result_json(d, utt_start, 0) prints"""
        need = self._L.ssw_recognition_set_json(self._r, u, float(utt_start), frate, None, 0)
        _check(need, "ssw_recognition_set_json")
        buf = C.create_string_buffer(need + 1)
        _check(self._L.ssw_recognition_set_json(self._r, u, float(utt_start), frate, buf, need + 1),
               "ssw_recognition_set_json")
        return buf.value.decode()

    def align(self, model: "Model", d_senscr, utt_off, stream=None) -> "AlignmentSet":
        """ssw_recognition_set_align: decoder_alignment (src/decoder.c:737-798) for every
        utterance of this set over whole rows in HBM -- the rows the search read (d_senscr device
        int16 [n_frames][n_sen]).  Status per utterance: 0 aligned, 1 no hypothesis (this set's
        message), 2 populate or the second pass failed."""
        off = np.ascontiguousarray(utt_off, np.int32)
        if len(off) - 1 != self.n_utts:
            raise SswError("ssw_recognition_set_align: utt_off is for %d utterances, the set has %d"
                           % (len(off) - 1, self.n_utts))
        h = self._L.ssw_recognition_set_align(model._m, self._r, _ptr(d_senscr), int(off[-1]),
                                              _ptr(off), _ptr(stream))
        if not h:
            raise SswError("ssw_recognition_set_align: " + _lib.last_error())
        return AlignmentSet(self._L, h, self._lex)

    def free(self):
        if getattr(self, "_r", None):
            self._L.ssw_recognition_set_free(self._r)
            self._r = None

    __del__ = free


def _fsg_of_utt(fsg_of_utt, n_utts):
    if fsg_of_utt is None:
        return None
    a = np.ascontiguousarray(fsg_of_utt, np.int32)
    assert len(a) == n_utts
    return a


def grammar_search_batch(model: Model, lex: Lexicon, d_senscr, utt_off, plan: GrammarPlan,
                         fsg_of_utt=None, stream=None) -> RecognitionSet:
    """ssw_grammar_search_batch: senone scores in HBM (compallsen = yes rows) -> recognition
    against the plan's grammars, utterance u against grammar fsg_of_utt[u] (None: grammar 0)."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    g = _fsg_of_utt(fsg_of_utt, n_utts)
    L = _lib.lib()
    h = L.ssw_grammar_search_batch(model._m, lex._d, plan._p, _ptr(g), _ptr(d_senscr),
                                   int(off[-1]), _ptr(off), n_utts, _ptr(stream))
    if not h:
        raise SswError("ssw_grammar_search_batch: " + _lib.last_error())
    return RecognitionSet(L, h, lex, n_utts)


def recognize_batch(model: Model, lex: Lexicon, d_feats, utt_off, plan: GrammarPlan,
                    fsg_of_utt=None, scorer=None, stream=None) -> RecognitionSet:
    """ssw_recognize_batch: feature rows in HBM -> all senone scores -> grammar search."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    g = _fsg_of_utt(fsg_of_utt, n_utts)
    L = _lib.lib()
    h = L.ssw_recognize_batch(model._m, lex._d, plan._p, _ptr(g), model.pick_scorer(scorer), _ptr(d_feats),
                              int(off[-1]), _ptr(off), n_utts, _ptr(stream))
    if not h:
        raise SswError("ssw_recognize_batch: " + _lib.last_error())
    return RecognitionSet(L, h, lex, n_utts)


def recognize_batch_active(model: Model, lex: Lexicon, d_feats, utt_off, plan: GrammarPlan,
                           fsg_of_utt=None, scorer=None, d_senscr=None, want_listed=False,
                           stream=None):
    """ssw_recognize_batch_active: recognition in the reference's DEFAULT configuration
    (compallsen = no) from feature rows in HBM.  Returns (RecognitionSet, rounds int32 [n_utts])
    and, with want_listed, the uint32 [n_frames][(n_sen + 31) / 32] bitmap of the listed senones
    of every frame (bridges included) as a third item.  d_senscr: optional device int16
    [n_frames][n_sen] that receives the rows as acmod's buffer would hold them."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    g = _fsg_of_utt(fsg_of_utt, n_utts)
    rounds = np.zeros(n_utts, np.int32)
    listed = np.zeros((int(off[-1]), (model.n_sen + 31) // 32), np.uint32) if want_listed else None
    L = _lib.lib()
    h = L.ssw_recognize_batch_active(model._m, lex._d, plan._p, _ptr(g),
                                     model.pick_scorer(scorer), _ptr(d_feats),
                                     int(off[-1]), _ptr(off), n_utts, _ptr(d_senscr),
                                     _ptr(listed), _ptr(rounds), _ptr(stream))
    if not h:
        raise SswError("ssw_recognize_batch_active: " + _lib.last_error())
    r = RecognitionSet(L, h, lex, n_utts)
    return (r, rounds, listed) if want_listed else (r, rounds)


def recognize_audio_batch(model: Model, lex: Lexicon, pcm, samp_off, plan: GrammarPlan,
                          fsg_of_utt=None, samprate=None, fe_cfg=None, scorer=None,
                          stream=None, active=False, pcm_format=None) -> RecognitionSet:
    """Audio in, hypotheses out: decoder_process_int16(full_utt) + decoder_hyp / decoder_seg_iter
    under decoder_set_fsg with compallsen = yes, for a batch.  int16 PCM (host array or device
    tensor; utterance u = samples samp_off[u] .. samp_off[u + 1]) -> ssw_fe_batch (samprate None:
    16 kHz) or ssw_fe_batch_ex -> ssw_feat_batch (ssw_feat_batch_ex when the model's
    feat_params.json asks for anything but the plain features) -> ssw_recognize_batch, or
    ssw_recognize_batch_active when active=True (the reference's default compallsen = no).
    float32 audio as align_audio_batch takes it (decoder_process_float32)."""
    width = model._audio_feat_width()
    audio = _AudioIn(model, pcm, samp_off, samprate, fe_cfg, pcm_format, "recognize_audio_batch")
    n_frames = audio.n_frames
    d_cep = model.device_malloc(n_frames * audio.ncep * 4) if n_frames else None
    d_feat = model.device_malloc(n_frames * width * 4) if n_frames else None
    try:
        fo = audio.cepstra(d_cep if d_cep else 0, stream)
        if n_frames:
            model._audio_feats(d_cep, n_frames, fo, d_feat, stream, audio.ncep)
        if active:
            return recognize_batch_active(model, lex, d_feat if d_feat else 0, fo, plan,
                                          fsg_of_utt, scorer=scorer, stream=stream)[0]
        return recognize_batch(model, lex, d_feat if d_feat else 0, fo, plan, fsg_of_utt,
                               scorer=scorer, stream=stream)
    finally:
        audio.free()
        for p in (d_cep, d_feat):
            if p:
                model.device_free(p)


def recognize_align_batch(model: Model, lex: Lexicon, d_feats, utt_off, plan: GrammarPlan,
                          fsg_of_utt=None, scorer=None, two_pass_history=False, stream=None):
    """ssw_recognize_align_batch: recognize_batch, then decoder_alignment (src/decoder.c:737-798)
    of what was recognised, over the same rows (compallsen = yes) -- what decoder_result_json
    prints at align_level 1 and 2 after a grammar.  two_pass_history: the rows are made again
    between the two searches from the top-N order each utterance's search left.  Returns
    (RecognitionSet, AlignmentSet); the recognition set is recognize_batch's."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    g = _fsg_of_utt(fsg_of_utt, n_utts)
    rec = C.c_void_p()
    L = _lib.lib()
    h = L.ssw_recognize_align_batch(model._m, lex._d, plan._p, _ptr(g), model.pick_scorer(scorer),
                                    _ptr(d_feats), int(off[-1]), _ptr(off), n_utts,
                                    int(bool(two_pass_history)), C.byref(rec), _ptr(stream))
    if not h:
        raise SswError("ssw_recognize_align_batch: " + _lib.last_error())
    return RecognitionSet(L, rec, lex, n_utts), AlignmentSet(L, h, lex)


def recognize_align_batch_active(model: Model, lex: Lexicon, d_feats, utt_off, plan: GrammarPlan,
                                 fsg_of_utt=None, scorer=None, two_pass_history=False,
                                 stream=None):
    """ssw_recognize_align_batch_active: recognize_align_batch in the reference's DEFAULT
    configuration (compallsen = no): the second pass scores for itself, its active set seeded
    with what the grammar search's last frame left.  Returns (RecognitionSet, AlignmentSet,
    rounds int32 [n_utts]); set and rounds are recognize_batch_active's."""
    off = np.ascontiguousarray(utt_off, np.int32)
    n_utts = len(off) - 1
    g = _fsg_of_utt(fsg_of_utt, n_utts)
    rounds = np.zeros(n_utts, np.int32)
    rec = C.c_void_p()
    L = _lib.lib()
    h = L.ssw_recognize_align_batch_active(model._m, lex._d, plan._p, _ptr(g),
                                           model.pick_scorer(scorer), _ptr(d_feats), int(off[-1]),
                                           _ptr(off), n_utts, int(bool(two_pass_history)),
                                           C.byref(rec), _ptr(rounds), _ptr(stream))
    if not h:
        raise SswError("ssw_recognize_align_batch_active: " + _lib.last_error())
    return RecognitionSet(L, rec, lex, n_utts), AlignmentSet(L, h, lex), rounds


def recognize_align_audio_batch(model: Model, lex: Lexicon, pcm, samp_off, plan: GrammarPlan,
                                fsg_of_utt=None, samprate=None, fe_cfg=None, scorer=None,
                                stream=None, active=False, two_pass_history=False,
                                pcm_format=None):
    """Audio in, hypotheses with phone and state times out: recognize_audio_batch followed by
    decoder_alignment, i.e. decoder_result_json(d, start, 1 or 2) after decoder_set_fsg /
    decoder_set_jsgf_*, for a batch.  The front end is recognize_audio_batch's; then
    ssw_recognize_align_batch, or ssw_recognize_align_batch_active when active=True (the
    reference's default compallsen = no).  Returns (RecognitionSet, AlignmentSet)."""
    width = model._audio_feat_width()
    audio = _AudioIn(model, pcm, samp_off, samprate, fe_cfg, pcm_format,
                     "recognize_align_audio_batch")
    n_frames = audio.n_frames
    d_cep = model.device_malloc(n_frames * audio.ncep * 4) if n_frames else None
    d_feat = model.device_malloc(n_frames * width * 4) if n_frames else None
    try:
        fo = audio.cepstra(d_cep if d_cep else 0, stream)
        if n_frames:
            model._audio_feats(d_cep, n_frames, fo, d_feat, stream, audio.ncep)
        fn = recognize_align_batch_active if active else recognize_align_batch
        return fn(model, lex, d_feat if d_feat else 0, fo, plan, fsg_of_utt, scorer=scorer,
                  two_pass_history=two_pass_history, stream=stream)[:2]
    finally:
        audio.free()
        for p in (d_cep, d_feat):
            if p:
                model.device_free(p)


# ---- voice activity detection and endpointing (vad.h, endpointer.h) ------------------------

VAD_STATE_DTYPE = np.dtype(_lib.SswVadState)
ENDPOINT_SEG_DTYPE = np.dtype(_lib.SswEndpointSeg)


def _vad_pcm_check(pcm, who):
    """int16 audio only: the reference's detector has no float entry, and what 1.0 should stand
    for is the caller's to say"""
    dt = str(pcm.dtype) if hasattr(pcm, "data_ptr") else np.asarray(pcm).dtype
    name = str(dt).replace("torch.", "")
    if "float" in name or "double" in name or name in ("half", "bfloat16"):
        raise SswError(f"{who}: audio of dtype {name}; the detector takes int16 samples, so "
                       "scale float audio yourself (e.g. x * 32768) and convert")
    if name != "int16":
        raise SswError(f"{who}: audio of dtype {name} (int16)")


def _vad_device_pcm(pcm, who):
    """the audio as a contiguous int16 device tensor (a host array is uploaded)"""
    import torch
    _vad_pcm_check(pcm, who)
    if _is_device_tensor(pcm):
        return pcm.contiguous().reshape(-1)
    host = pcm.numpy() if hasattr(pcm, "data_ptr") else np.asarray(pcm)
    return torch.from_numpy(np.ascontiguousarray(host, np.int16).reshape(-1)).to("cuda")


class Vad:
    """vad_t for batches of streams: vad_init + vad_set_input_params (src/ps_vad.c:49-128), with
    vad_classify over every whole frame of every stream as one call.  mode 0..3 (loose to
    strict); sample_rate 0 = 16000; frame_length 0 = 0.03."""

    def __init__(self, mode=0, sample_rate=16000, frame_length=0.03):
        self._L = _lib.lib()
        self._h = self._L.ssw_vad_create(int(mode), int(sample_rate), float(frame_length))
        if not self._h:
            raise SswError("ssw_vad_create: " + _lib.last_error())
        self.mode = int(mode)
        self.frame_size = int(self._L.ssw_vad_frame_size(self._h))
        self.frame_length = float(self._L.ssw_vad_frame_length(self._h))
        self.sample_rate = int(self._L.ssw_vad_sample_rate(self._h))
        self.closest_rate = int(self._L.ssw_vad_closest_rate(self._h))

    def frame_count(self, n_samples) -> int:
        return int(_check(int(self._L.ssw_vad_frame_count(self._h, int(n_samples))),
                          "ssw_vad_frame_count"))

    def set_streams_per_workgroup(self, streams=0):
        """ssw_vad_set_streams_per_workgroup: 8, 16, 32 or 64 of a workgroup's lanes take streams;
        0 = by the batch's size.  The results do not depend on it."""
        _check(self._L.ssw_vad_set_streams_per_workgroup(self._h, int(streams)),
               "ssw_vad_set_streams_per_workgroup")

    def new_states(self, n) -> np.ndarray:
        """n states as WebRtcVad_InitCore leaves them (VAD_STATE_DTYPE); np.zeros of that dtype
        is n states not yet set up, which a batch call starts afresh too"""
        s = np.zeros(int(n), VAD_STATE_DTYPE)
        for i in range(len(s)):
            self._L.ssw_vad_state_init(C.c_void_p(s[i:i + 1].ctypes.data))
        return s

    @staticmethod
    def _state_arg(state, n):
        if state is None:
            return None
        if not (isinstance(state, np.ndarray) and state.dtype == VAD_STATE_DTYPE
                and state.shape == (n,) and state.flags.c_contiguous):
            raise SswError("state: a contiguous numpy array [n_streams] of VAD_STATE_DTYPE")
        return state

    def classify_batch(self, pcm, samp_off, state=None, stream=None):
        """ssw_vad_batch: int16 audio (numpy array or device tensor), stream u = samples
        samp_off[u] .. samp_off[u + 1] -> (is_speech int8 [total frames] on the host, frame_off
        int32 [n + 1]).  state: None, or Vad.new_states(n), updated in place."""
        off = np.ascontiguousarray(samp_off, np.int64)
        n = len(off) - 1
        import torch
        d_pcm = _vad_device_pcm(pcm, "Vad.classify_batch")
        if n >= 0 and len(off) and int(off[-1]) > d_pcm.numel():
            raise SswError("Vad.classify_batch: samp_off runs past the audio")
        frame_off = np.zeros(n + 1, np.int32)
        total = int((np.diff(off) // self.frame_size).sum()) if n > 0 else 0
        d_out = torch.empty(max(total, 1), dtype=torch.int8, device=d_pcm.device)
        st = self._state_arg(state, n)
        _check(self._L.ssw_vad_batch(self._h, _ptr(d_pcm), _ptr(off), n, _ptr(d_out),
                                     _ptr(frame_off), _ptr(st), _ptr(stream)), "ssw_vad_batch")
        return d_out[:total].cpu().numpy(), frame_off

    def classify_batch_host(self, pcm, samp_off, state=None, features=False):
        """ssw_vad_batch_host: the same on the host, from the same arithmetic source; with
        features=True also the int16 [frames][7] rows ssw_vad_debug_features shows"""
        _vad_pcm_check(pcm, "Vad.classify_batch_host")
        host = np.ascontiguousarray(pcm.cpu().numpy() if hasattr(pcm, "data_ptr") else pcm,
                                    np.int16).reshape(-1)
        off = np.ascontiguousarray(samp_off, np.int64)
        n = len(off) - 1
        if len(off) and int(off[-1]) > len(host):
            raise SswError("Vad.classify_batch_host: samp_off runs past the audio")
        frame_off = np.zeros(n + 1, np.int32)
        total = int((np.diff(off) // self.frame_size).sum()) if n > 0 else 0
        out = np.zeros(max(total, 1), np.int8)
        feat = np.zeros((max(total, 1), 7), np.int16) if features else None
        st = self._state_arg(state, n)
        _check(self._L.ssw_vad_batch_host(self._h, _ptr(host), _ptr(off), n, _ptr(out),
                                          _ptr(frame_off), _ptr(st), _ptr(feat)),
               "ssw_vad_batch_host")
        return (out[:total], frame_off, feat[:total]) if features else (out[:total], frame_off)

    def debug_features(self, n_frames) -> np.ndarray:
        """ssw_vad_debug_features of the last classify_batch: int16 [n_frames][7]"""
        out = np.zeros((max(int(n_frames), 1), 7), np.int16)
        _check(self._L.ssw_vad_debug_features(self._h, _ptr(out), int(n_frames)),
               "ssw_vad_debug_features")
        return out[:int(n_frames)]

    def endpoints_from_decisions(self, is_speech, tail_samples=0, window=0.3, ratio=0.9):
        """ssw_endpoints_from_decisions: the segments (ENDPOINT_SEG_DTYPE) of one stream"""
        dec = np.ascontiguousarray(is_speech, np.int8)
        h = self._L.ssw_endpoints_from_decisions(self._h, float(window), float(ratio), _ptr(dec),
                                                 len(dec), int(tail_samples))
        if not h:
            raise SswError("ssw_endpoints_from_decisions: " + _lib.last_error())
        try:
            return _endpoint_segments(self._L, h, 0)
        finally:
            self._L.ssw_endpoints_free(h)

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.ssw_vad_free(self._h)
            self._h = None


def _endpoint_segments(L, h, u) -> np.ndarray:
    n = L.ssw_endpoints_count(h, u)
    if n < 0:
        raise SswError("ssw_endpoints_count: no such stream")
    segs = np.zeros(n, ENDPOINT_SEG_DTYPE)
    for k in range(n):
        _check(L.ssw_endpoints_get(h, u, k, C.cast(C.c_void_p(segs[k:k + 1].ctypes.data),
                                                   C.POINTER(_lib.SswEndpointSeg))),
               "ssw_endpoints_get")
    return segs


class Endpoints:
    """What endpoint_audio_batch found: per stream the utterances endpointer_process and
    endpointer_end_stream hand back (src/ps_endpointer.c:233-322)."""

    def __init__(self, vad: Vad, d_pcm, samp_off, segments):
        self.vad = vad
        self._d_pcm = d_pcm
        self._off = samp_off
        self._segs = segments

    def __len__(self):
        return len(self._segs)

    def segments(self, u) -> np.ndarray:
        """stream u's segments, ENDPOINT_SEG_DTYPE: first_sample (in the stream), n_samples,
        speech_start, speech_end (seconds)"""
        return self._segs[u]

    def utterances(self):
        """(pcm, samp_off, stream_of_utt, start_time): every segment's samples gathered into one
        int16 device tensor, ready for align_audio_batch / recognize_audio_batch"""
        import torch
        stream_of = np.concatenate([np.full(len(s), u, np.int32) for u, s in enumerate(self._segs)]
                                   + [np.zeros(0, np.int32)])
        first = np.concatenate([self._off[u] + s["first_sample"] for u, s in enumerate(self._segs)]
                               + [np.zeros(0, np.int64)]).astype(np.int64)
        lens = np.concatenate([s["n_samples"] for s in self._segs]
                              + [np.zeros(0, np.int64)]).astype(np.int64)
        start = np.concatenate([s["speech_start"] for s in self._segs] + [np.zeros(0)])
        off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        dev = self._d_pcm.device
        shift = torch.from_numpy(first - off[:-1]).to(dev)
        idx = torch.arange(int(off[-1]), device=dev) + torch.repeat_interleave(
            shift, torch.from_numpy(lens).to(dev))
        return self._d_pcm[idx], off, stream_of, start


def endpoint_audio_batch(pcm, samp_off, samprate=16000, mode=0, window=0.3, ratio=0.9,
                         frame_length=0.03, stream=None) -> Endpoints:
    """ssw_endpoint_batch: a fresh endpointer_init(window, ratio, mode, samprate, frame_length)
    per stream over all of its audio -- endpointer_process on every whole frame, then
    endpointer_end_stream with the samples left over.  int16 audio, numpy array or device
    tensor; stream u = samples samp_off[u] .. samp_off[u + 1]."""
    vad = Vad(mode, samprate, frame_length)
    L = vad._L
    off = np.ascontiguousarray(samp_off, np.int64)
    d_pcm = _vad_device_pcm(pcm, "endpoint_audio_batch")
    if len(off) and int(off[-1]) > d_pcm.numel():
        raise SswError("endpoint_audio_batch: samp_off runs past the audio")
    h = L.ssw_endpoint_batch(vad._h, float(window), float(ratio), _ptr(d_pcm), _ptr(off),
                             len(off) - 1, _ptr(stream))
    if not h:
        raise SswError("ssw_endpoint_batch: " + _lib.last_error())
    try:
        segs = [_endpoint_segments(L, h, u) for u in range(len(off) - 1)]
    finally:
        L.ssw_endpoints_free(h)
    return Endpoints(vad, d_pcm, off, segs)
