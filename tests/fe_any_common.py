"""What tests/golden/make_fe_any.py records and the tests of the front end under any settings
replay: the fixtures of tests/golden/fe_any_mfcc.npz ("cep/<name>": the reference's rows, float32
[frames][ncep, or nfilt with logspec / smoothspec]) and of fe_any_align.json
("<compallsen>": decoder_result_json at level 1 on a model directory with changed settings).

Inputs are made from goforward.raw with integer arithmetic (fe_rates_common.resample) and, for
float32 samples, IEEE float32 / on integer-valued arrays, so no audio is committed.  Unless a
fixture says otherwise it uses the en-us model's settings at 16 kHz on the first 1.5 s, which
is 149 frames."""
import json
import os

import numpy as np

from tests import fe_rates_common as R

GOLD = R.GOLD
MFCC_NPZ = os.path.join(GOLD, "fe_any_mfcc.npz")
ALIGN_JSON = os.path.join(GOLD, "fe_any_align.json")
MODEL_EN = os.path.join(R.ROOT, "soundswallower_amd", "model", "en-us")

SECONDS = 1.5
WIDE = {"nfilt": 40, "lowerf": 133.33334, "upperf": 6855.4976}

# the settings the alignment fixture's model directory declares besides en-us's own
ALIGN_SETTINGS = {"remove_dc": True, "round_filters": False, "alpha": 0.95}
ALIGN_TEXT = R.ALIGN_TEXT
CONFIGS = ("yes", "no")                      # compallsen

_F = np.float32


def _f32(x, div):
    return np.asarray(x, np.int64).astype(np.float32) / _F(div)


# sample kind -> (the driver's KIND, int16 samples -> what the front end is given)
KINDS = {
    "i16": ("i16", lambda x: x),
    # sample values that are not whole numbers: x / 3 (1.0 stands for 32768; / 32768 is exact)
    "f32_third": ("f32", lambda x: _f32(x, 3) / _F(32768)),
    # exactly the int16 audio
    "f32_exact": ("f32", lambda x: _f32(x, 32768)),
}


def _fixtures():
    """(name, rate, settings over en-us's ("warp_type" and "warp_params" among them), input,
    sample kind); input: ("head", n or None for 1.5 s) or ("offset", d): 1.5 s with d added to
    every sample, clipped"""
    fx = []

    def add(name, cfg, rate=16000, pcm=("head", None), kind="i16"):
        fx.append((name, rate, cfg, pcm, kind))

    add("remove_dc", {"remove_dc": True})
    add("alpha095", {"alpha": 0.95})
    add("alpha0", {"alpha": 0.0})
    add("htk_l22", {"transform": "htk", "lifter": 22})
    for n in (1, 12, 20, 26):
        add(f"ncep{n}", {"ncep": n})
    add("logspec_n1", {"logspec": True, "remove_noise": True, "lifter": 0})
    add("logspec_n0", {"logspec": True, "remove_noise": False, "lifter": 0})
    add("smoothspec_f20", {"smoothspec": True})
    add("smoothspec_f40", dict(WIDE, smoothspec=True))
    add("logspec_l22", {"logspec": True, "lifter": 22})
    add("doublebw", {"doublebw": True})
    add("doublebw_300_3400", {"doublebw": True, "lowerf": 300.0, "upperf": 3400.0})
    add("unit_area_no", {"unit_area": False})
    add("round_filters_no", {"round_filters": False})
    add("warp_inverse_linear", {"warp_type": "inverse_linear", "warp_params": "1.1"})
    add("warp_affine", {"warp_type": "affine", "warp_params": "1.05 20"})
    add("warp_piecewise_linear", {"warp_type": "piecewise_linear", "warp_params": "0.9 3000"})
    add("combo8000", {"lowerf": 1.0, "upperf": 4000.0, "nfilt": 20, "round_filters": False,
                      "remove_dc": True, "wlen": 0.0256, "remove_noise": False}, rate=8000)
    # remove_dc's edges
    add("dc_offset900", {"remove_dc": True}, pcm=("offset", 900))
    for n in (1, 409, 410, 411, 569, 570, 571):
        add(f"dc_len{n}", {"remove_dc": True}, pcm=("head", n))
    add("dc_192000_alpha0001", {"remove_dc": True, "alpha": 0.001}, rate=192000)
    add("dc_f32_third", {"remove_dc": True}, kind="f32_third")
    add("dc_f32_exact", {"remove_dc": True}, kind="f32_exact")
    return fx


FIXTURES = _fixtures()


def int_pcm(spec, rate):
    y = R.goforward() if rate == 16000 else R.resample(R.goforward(), rate)
    whole = int(SECONDS * rate)
    if spec[0] == "head":
        return y[:whole if spec[1] is None else spec[1]].copy()
    if spec[0] == "offset":
        return (y[:whole].astype(np.int32) + spec[1]).clip(-32768, 32767).astype(np.int16)
    raise ValueError(spec)


def fixture_pcm(fx):
    """the samples the front end is given: int16, or float32 for the f32 kinds"""
    _, rate, _, spec, kind = fx
    return KINDS[kind][1](int_pcm(spec, rate))


def settings(cfg):
    """en-us's front-end settings with cfg's overrides, the warp strings apart:
    (settings, warp_type or None, warp_params or None)"""
    s = dict(R.EN_US)
    s.update(cfg)
    return s, s.pop("warp_type", None), s.pop("warp_params", None)


def reference_json(cfg, rate):
    """the settings as the reference's config_parse_json takes them"""
    s = dict(R.EN_US)
    s.update(cfg)
    s["samprate"] = int(rate)
    return json.dumps(s)


def align_model_dir(path):
    """en-us with ALIGN_SETTINGS in its feat_params.json, as a directory of links at `path`"""
    os.makedirs(path)
    for f in os.listdir(MODEL_EN):
        if f != "feat_params.json":
            os.symlink(os.path.join(MODEL_EN, f), os.path.join(path, f))
    with open(os.path.join(MODEL_EN, "feat_params.json")) as f:
        params = json.load(f)
    params.update(ALIGN_SETTINGS)
    with open(os.path.join(path, "feat_params.json"), "w") as f:
        json.dump(params, f)
    return path
