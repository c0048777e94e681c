"""What tests/golden/make_mfcc_rates.py records and the front-end tests at other sample rates
replay: goforward resampled from 16 kHz with integer arithmetic only (so the PCM is the same on
every machine and none of it is committed), and the list of fixtures in
tests/golden/fe_rates_mfcc.npz with their settings and inputs."""
import json
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MFCC_NPZ = os.path.join(GOLD, "fe_rates_mfcc.npz")
ALIGN_JSON = os.path.join(GOLD, "fe_rates_align.json")

RATES = (8000, 11025, 16000, 22050, 32000, 44100, 48000, 96000, 192000)
ALIGN_RATES = (44100, 8000)
ALIGN_TEXT = "go forward ten meters"

# the en-us model's front-end settings (model/en-us/feat_params.json)
EN_US = {"lowerf": 130.0, "upperf": 3700.0, "nfilt": 20, "transform": "dct", "lifter": 22,
         "remove_noise": True}


def goforward():
    return np.fromfile(os.path.join(GOLD, "goforward.raw"), dtype="<i2")


def resample(x, rate):
    """x at 16 kHz -> rate Hz by linear interpolation in integers: sample n of the output lies at
    i + r / rate input samples, i, r = divmod(16000 n, rate); y[n] = (x[i] (rate - r) +
    x[i + 1] r) // rate, holding the last sample"""
    x = np.asarray(x, np.int64)
    n_out = len(x) * rate // 16000
    i, r = np.divmod(np.arange(n_out, dtype=np.int64) * 16000, rate)
    nxt = np.minimum(i + 1, len(x) - 1)
    return ((x[i] * (rate - r) + x[nxt] * r) // rate).astype(np.int16)


def framing(rate, frate=100, wlen=0.025625):
    """(frame shift, frame size) as fe_init computes them, in float32"""
    sr = np.float32(rate)
    return (int(float(sr / np.float32(frate)) + 0.5), int(float(sr * np.float32(wlen)) + 0.5))


def _fixtures():
    fx = []
    for r in RATES:                                    # the model's settings, automatic nfft
        fx.append((f"rate{r}", r, {}, ("go",)))
    for n in (2048, 4096):
        fx.append((f"rate44100_nfft{n}", 44100, {"nfft": n}, ("go",)))
    # the small FFTs: 64 and 128 points at 8 kHz
    fx.append(("rate8000_nfft64", 8000, {"wlen": 0.008, "frate": 200, "nfilt": 5, "lowerf": 130.0,
                                         "upperf": 3700.0}, ("go",)))
    fx.append(("rate8000_nfft128", 8000, {"wlen": 0.016, "nfilt": 8}, ("go",)))
    for transform in ("dct", "legacy"):
        for noise in (True, False):
            for lifter in (0, 22):
                for nfilt in (20, 40):
                    lo, hi = (130.0, 3700.0) if nfilt == 20 else (133.33334, 6855.4976)
                    cfg = {"transform": transform, "remove_noise": noise, "lifter": lifter,
                           "nfilt": nfilt, "lowerf": lo, "upperf": hi}
                    fx.append((f"cfg44100_{transform}_n{int(noise)}_l{lifter}_f{nfilt}", 44100,
                               cfg, ("piece", 66150)))          # 1.5 s
    fx.append(("rate22050_frate80_wlen32", 22050, {"frate": 80, "wlen": 0.032}, ("go",)))
    fx.append(("rate8000_upperf4001", 8000, {"upperf": 4001.0}, ("go",)))
    for r in (11025, 44100):
        shift, size = framing(r)
        for n in (1, size - 1, size, size + 1, size + shift - 1, size + shift, size + shift + 1):
            fx.append((f"edge{r}_{n}", r, {}, ("piece", n)))
    fx.append(("long48000", 48000, {}, ("tile", 30 * 48000)))  # 30 s: the noise tracker's recurrence
    return fx


FIXTURES = _fixtures()


def fixture_pcm(spec, rate):
    y = resample(goforward(), rate)
    if spec[0] == "go":
        return y
    if spec[0] == "piece":
        return y[:spec[1]].copy()
    if spec[0] == "tile":
        return np.tile(y, spec[1] // len(y) + 1)[:spec[1]].copy()
    raise ValueError(spec)


def settings(cfg):
    """the model's front-end settings with cfg's overrides"""
    s = dict(EN_US)
    s.update(cfg)
    return s


def reference_json(cfg, rate):
    """the settings as the reference's config_parse_json takes them"""
    s = settings(cfg)
    s["samprate"] = int(rate)
    s["remove_noise"] = bool(s["remove_noise"])
    return json.dumps(s)


def count_limit(rate):
    """frame counts are recorded for n = 1 .. size + 3 shift"""
    shift, size = framing(rate)
    return size + 3 * shift
