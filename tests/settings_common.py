"""The cases of the non-default logbase / varfloor / mixwfloor / tmatfloor pins, named once for
the recorder (tests/golden/make_settings.py) and for the tests (tests/test_settings_host.py,
tests/test_gpu_settings.py).

A case is a model and the settings that leave their defaults.  The models:

  en-us    the shipped model (the reference scores it with ptm)
  fr-mixw  fr-fr with the mixture_weights file tests/test_cabi_host.synth_mixw_from_sendump makes
           of its sendump, and no sendump (the reference scores it with ptm too: its mixture
           weights quantised from the file's floats, under mixwfloor); made in a directory
           the caller names

The fixture keeps, per scoring case, what tests/golden/make_cont.py keeps (scorer, det_crc,
var_crc, frames, row_crc, the whole rows of frames 0, 1, 2 and the last) and the count of floored
variances the reference logs; per flow case the decoder's JSON, hypothesis, score and segments.
"""
from __future__ import annotations

import json
import os
import shutil
import zlib

import numpy as np

from tests import sc_common as S

ROOT = S.ROOT
GOLD = S.GOLD
EN_US = S.EN_US
FR_FR = os.path.join(ROOT, "soundswallower_amd", "model", "fr-fr")
RESULTS_JSON = os.path.join(GOLD, "settings_results.json")
ROWS_NPZ = os.path.join(GOLD, "settings", "rows.npz")
PCM = os.path.join(GOLD, "goforward.raw")
FSG = os.path.join(GOLD, "fsg", "goforward.fsg")
FEAT_EN = S.FEAT_A                                           # en-us's front end on goforward.raw
FEAT_FR = os.path.join(GOLD, "mllr", "goforward_fr_feat.npy")  # fr-fr's
TEXT = ["go", "forward", "ten", "meters"]
DEFAULTS = {"logbase": 1.0001, "varfloor": 1e-4, "mixwfloor": 1e-7, "tmatfloor": 1e-4}
KEYS = ("logbase", "varfloor", "mixwfloor", "tmatfloor")

# the 8-bit log-add table by base: (largest entry T, last non-zero index or None, entries or
# None where the loader refuses).  Computed from build_logadd8's formula before any test ran.
LOGADD_ROWS = {
    1.00001: (68, 255, 515),
    1.000015: (45, 255, 317),
    1.000018: (38, 254, 256),
    1.00003: (23, 135, 256),
    1.00005: (14, 71, 256),
    1.0001: (7, 28, 256),
    1.0003: (2, 5, 256),
    1.001: (1, 0, 256),
    1.003: (0, None, 256),
}
LOGBASE_REFUSED_AT_LOAD = 1.000002
# the reference's table has more than 256 entries there and its log-add reads them all
LOGBASES_REFUSED_AT_SCORING = (1.00001, 1.000015)
LOGBASES_ACCEPTED = (1.000018, 1.00003, 1.00005, 1.0001, 1.0003, 1.001, 1.003)

# scoring cases recorded from the reference: name -> (model, the settings that are not default)
SCORING = {
    "logbase_1.000018": ("en-us", {"logbase": 1.000018}),
    "logbase_1.00003": ("en-us", {"logbase": 1.00003}),
    "logbase_1.0003": ("en-us", {"logbase": 1.0003}),
    "logbase_1.003": ("en-us", {"logbase": 1.003}),
    "varfloor_1e-2": ("en-us", {"varfloor": 1e-2}),
    "varfloor_1": ("en-us", {"varfloor": 1.0}),
    "mixwfloor_1e-3": ("fr-mixw", {"mixwfloor": 1e-3}),
    "mixwfloor_0.05": ("fr-mixw", {"mixwfloor": 0.05}),
}
# flows: name -> (kind, model, settings)
FLOWS = {
    "align_logbase_1.0003": ("align", "en-us", {"logbase": 1.0003}),
    "align_tmatfloor_1e-2": ("align", "en-us", {"tmatfloor": 1e-2}),
    "align_tmatfloor_0.3": ("align", "en-us", {"tmatfloor": 0.3}),
    # (1e-2 is below every non-zero probability of en-us's matrices and changes none of them; 0.1
    # raises the two smallest, 0.055 and 0.083)
    "align_tmatfloor_0.1": ("align", "en-us", {"tmatfloor": 0.1}),
    "rec_logbase_1.0003": ("rec", "en-us", {"logbase": 1.0003}),
    # TEXT's chain grammar (chain_fsg), the grammar oracle/fsg_oracle.py restates the search of
    "rec_chain_logbase_1.0003": ("rec_chain", "en-us", {"logbase": 1.0003}),
    "rec_chain_default": ("rec_chain", "en-us", {}),
}


def chain_fsg(path):
    """TEXT as a grammar file: state i --word i, probability 1--> state i + 1, what
    decoder_set_align_text builds of the text"""
    lines = ["FSG_BEGIN chain", "NUM_STATES %d" % (len(TEXT) + 1), "START_STATE 0",
             "FINAL_STATE %d" % len(TEXT)]
    lines += ["TRANSITION %d %d 1.0 %s" % (i, i + 1, w) for i, w in enumerate(TEXT)]
    with open(path, "w", encoding="utf-8") as fh:
        fh.write("\n".join(lines + ["FSG_END"]) + "\n")
    return path


def settings(over):
    return dict(DEFAULTS, **over)


def fr_mixw_dir(d, orc_fr=None):
    """fr-fr's files with the synthesised mixture_weights and no sendump, in directory d"""
    from tests.test_cabi_host import synth_mixw_from_sendump
    if orc_fr is None:
        from oracle import oracle as O
        orc_fr = O.Model(FR_FR)
    os.makedirs(d, exist_ok=True)
    for n in ("mdef", "means", "variances", "transition_matrices", "dict.txt", "noisedict.txt",
              "feat_params.json"):
        shutil.copyfile(os.path.join(FR_FR, n), os.path.join(d, n))
    synth_mixw_from_sendump(orc_fr, os.path.join(d, "mixture_weights"))
    return d


def model_kwargs(model, fr_dir=None):
    """keyword arguments (but config) of soundswallower_amd.Model and, with `variances` renamed
    `vars`, of oracle.Model"""
    d = EN_US if model == "en-us" else fr_dir
    kw = dict(mdef=os.path.join(d, "mdef"), means=os.path.join(d, "means"),
              variances=os.path.join(d, "variances"), tmat=os.path.join(d, "transition_matrices"))
    if model == "en-us":
        kw["sendump"] = os.path.join(d, "sendump")
    else:
        kw["mixw"] = os.path.join(d, "mixture_weights")
    return kw


def load(model, over, device, fr_dir=None, **more):
    import soundswallower_amd as ssw
    cfg = dict(over, **more)
    if device is not None:
        cfg["device"] = device
    return ssw.Model(config=cfg, **model_kwargs(model, fr_dir))


def load_oracle(model, over, fr_dir=None):
    from oracle import oracle as O
    kw = model_kwargs(model, fr_dir)
    kw["vars"] = kw.pop("variances")
    return O.Model(config=dict(over), **kw)


def features(model):
    """the feature rows the reference scored for goforward.raw with the model's front end"""
    return np.load(FEAT_EN if model == "en-us" else FEAT_FR)


def floored_density_features(varfloor, n, seed):
    """n feature rows of en-us, each stream at the mean of a density that has a variance below
    `varfloor`, plus noise of 0.1 (scores are relative to the codebook's best density, so a frame
    exactly at a mean does not feel the floor; at 0.1 off, a dimension floored at 1e-4 costs 50
    natural-log units and one floored at 1e-2 half a unit): the floored densities then decide the
    top-N, which on the reference's recording they hardly do"""
    _, _, means = S.read_gauss(os.path.join(EN_US, "means"))
    _, _, var = S.read_gauss(os.path.join(EN_US, "variances"))
    rng = np.random.default_rng(seed)
    out = np.empty((n, 39), np.float32)
    floored = 0
    for f in range(3):
        cb, d = np.nonzero((var[f] < np.float32(varfloor)).any(axis=2))
        if len(cb) == 0:   # (a stream without such a variance: any density)
            cb, d = np.nonzero(np.ones(var[f].shape[:2], bool))
        else:
            floored += 1
        pick = rng.integers(0, len(cb), n)
        out[:, 13 * f:13 * f + 13] = means[f][cb[pick], d[pick]] \
            + (rng.standard_normal((n, 13)) * 0.1).astype(np.float32)
    assert floored > 0
    return np.ascontiguousarray(out)


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes()) & 0xFFFFFFFF


def row_crcs(rows):
    return S.row_crcs(rows)


def split_rows(got):
    return S.split_rows(got)


def results():
    """the fixture, the whole rows back in place: scoring.<case>.rows = {frame: [n_sen]}"""
    with open(RESULTS_JSON, encoding="utf-8") as fh:
        fx = json.load(fh)
    with np.load(ROWS_NPZ) as z:
        for case, rec in fx["scoring"].items():
            rec["rows"] = {t: z["%s/%s" % (case, t)].tolist() for t in rec["rows"]}
    return fx


def logadd_properties(tab):
    """(largest entry, last non-zero index or None) of a log-add table's first 256 entries"""
    tab = np.asarray(tab, np.int64)[:256]
    nz = np.flatnonzero(tab)
    return int(tab.max()), (int(nz[-1]) if len(nz) else None)
