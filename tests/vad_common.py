"""What tests/golden/make_vad.py records from the reference's vad.h and endpointer.h and the
voice activity tests replay: tests/golden/vad_results.npz ("dec/<case>": vad_classify's value per
frame, int8) and tests/golden/vad_endpoints.json ("segments": {case: [[first_sample, n_samples,
speech_start, speech_end], ...]} with the times as 17-digit strings; "refusals": {case: the
reference's message}).

No audio is committed beyond the two recordings the other tests use.  Every input is made from
them with integer arithmetic: padded to at least 400 frames of 30 ms by tiling with stretches of
low-level noise from a fixed-seed integer generator (the minimum tracker evicts values older than
100 frames, so a short stream never reaches that code), and brought to the other rates by
fe_rates_common.resample's integer linear interpolation."""
import os

import numpy as np

from tests import fe_rates_common as R

GOLD = R.GOLD
RESULTS_NPZ = os.path.join(GOLD, "vad_results.npz")
ENDPOINTS_JSON = os.path.join(GOLD, "vad_endpoints.json")

MODES = (0, 1, 2, 3)
RATES = (8000, 16000, 32000, 48000, 44100, 22050, 11025)
CLOSEST = {8000: 8000, 16000: 16000, 32000: 32000, 48000: 48000, 44100: 48000, 22050: 16000,
           11025: 8000}
FRAME_LENGTHS = (0.01, 0.02, 0.03)
RECORDINGS = ("goforward", "goforward_fr")
DEGENERATE = ("silence", "square", "noise3", "dc8000")
# 400 of the longest frames there are, 1440 samples of 44.1 kHz audio (32.7 ms), and a little more
MIN_SAMPLES_16K = 400 * 1440 * 16000 // 44100 + 3000
NOISE_SAMPLES_16K = 24000                       # 1.5 s between two copies of the recording
NOISE_AMPLITUDE = 20
DEGENERATE_SAMPLES_16K = 130 * 480              # past the tracker's 100 frames at 30 ms


def _lcg(n, seed):
    """n values of a 31-bit linear congruential generator (the constants of glibc's TYPE_0
    rand), as int64"""
    out = np.empty(n, np.int64)
    x = seed
    for i in range(n):
        x = (x * 1103515245 + 12345) & 0x7FFFFFFF
        out[i] = x
    return out


_CACHE = {}


def noise(n, amplitude, seed):
    """n samples uniform on -amplitude .. amplitude"""
    return ((_lcg(n, seed) >> 8) % (2 * amplitude + 1) - amplitude).astype(np.int16)


def recording16(name):
    """the input at 16 kHz, int16"""
    if ("16k", name) in _CACHE:
        return _CACHE["16k", name]
    if name in RECORDINGS:
        x = np.fromfile(os.path.join(GOLD, name + ".raw"), dtype="<i2")
        gap = noise(NOISE_SAMPLES_16K, NOISE_AMPLITUDE, 4242 + len(name))
        parts, total = [], 0
        while total < MIN_SAMPLES_16K:
            parts += [x, gap]
            total += len(x) + len(gap)
        y = np.concatenate(parts)
    elif name == "silence":
        y = np.zeros(DEGENERATE_SAMPLES_16K, np.int16)
    elif name == "square":                       # full scale, 16 samples up, 16 down
        y = np.where((np.arange(DEGENERATE_SAMPLES_16K) // 16) % 2 == 0, 32767, -32767).astype(np.int16)
    elif name == "noise3":
        y = noise(DEGENERATE_SAMPLES_16K, 3, 99)
    elif name == "dc8000":
        y = np.full(DEGENERATE_SAMPLES_16K, 8000, np.int16)
    else:
        raise ValueError(name)
    _CACHE["16k", name] = y
    return y


def stream(name, rate):
    """the input at rate Hz"""
    key = (rate, name)
    if key not in _CACHE:
        y = recording16(name)
        _CACHE[key] = y if rate == 16000 else R.resample(y, rate)
    return _CACHE[key]


def frame_size(rate, frame_length):
    return int(CLOSEST[rate] * frame_length)


def _ms(frame_length):
    return int(round(frame_length * 1000))


def _vad_cases():
    """(case, input, mode, rate, frame_length): every rate with every frame length in the loosest
    and the strictest mode, the two modes between at 30 ms; the degenerate inputs at the four
    rates the detector works at (30 ms, modes 0 and 3) and at 16 kHz with every frame length"""
    cases = []
    for rate in RATES:
        for fl in FRAME_LENGTHS:
            for mode in MODES:
                if mode in (1, 2) and fl != 0.03:
                    continue
                for rec in RECORDINGS:
                    cases.append((f"{rec}_r{rate}_m{mode}_f{_ms(fl)}", rec, mode, rate, fl))
    for name in DEGENERATE:
        for rate in (8000, 16000, 32000, 48000):
            for mode in (0, 3):
                cases.append((f"{name}_r{rate}_m{mode}_f30", name, mode, rate, 0.03))
        for fl in (0.01, 0.02):
            cases.append((f"{name}_r16000_m0_f{_ms(fl)}", name, 0, 16000, fl))
    return cases


VAD_CASES = _vad_cases()
SPEECH_CASES = [c for c in VAD_CASES if c[1] in RECORDINGS]

WINDOWS = ((0.3, 0.9), (0.5, 0.8))
TRAILING = ("0", "1", "size-1")


def ep_stream(name, rate, frame_length, trailing):
    """the recording cut in the middle of its second copy of the speech -- so that the stream
    ends inside an utterance and endpointer_end_stream has samples to hand back -- at a length
    that leaves `trailing` samples after the last whole frame"""
    y = stream(name, rate)
    size = frame_size(rate, frame_length)
    rec = len(np.fromfile(os.path.join(GOLD, name + ".raw"), dtype="<i2"))
    cut16 = rec + NOISE_SAMPLES_16K + rec // 2
    cut = cut16 * rate // 16000
    t = {"0": 0, "1": 1, "size-1": size - 1}[trailing]
    return y[:cut - cut % size + t]


def _ep_cases():
    """(case, input, mode, rate, frame_length, window, ratio, trailing or None for the whole
    padded recording)"""
    cases = []
    for (window, ratio) in WINDOWS:
        tag = f"w{int(window * 10)}"
        for rec in RECORDINGS:
            for (rate, fl, mode) in ((16000, 0.03, 0), (16000, 0.01, 3), (44100, 0.02, 1),
                                     (8000, 0.03, 2), (48000, 0.03, 0)):
                cases.append((f"{rec}_r{rate}_m{mode}_f{_ms(fl)}_{tag}", rec, mode, rate, fl,
                              window, ratio, None))
        for trailing in TRAILING:
            for (rate, fl) in ((16000, 0.03), (22050, 0.02)):
                cases.append((f"goforward_r{rate}_m0_f{_ms(fl)}_{tag}_t{trailing}", "goforward", 0,
                              rate, fl, window, ratio, trailing))
    return cases


EP_CASES = _ep_cases()


def ep_input(case):
    _, name, _, rate, fl, _, _, trailing = case
    return stream(name, rate) if trailing is None else ep_stream(name, rate, fl, trailing)


# (case, "vad" or "ep", arguments in the order of the reference's init)
REFUSALS = (
    ("rate100000", "vad", (0, 100000, 0.03)),
    ("frame_length_0.015", "vad", (0, 16000, 0.015)),
    ("mode4", "vad", (4, 16000, 0.03)),
    ("ratio_0.999", "ep", (0.3, 0.999, 0, 16000, 0.03)),
    ("ratio_0.05", "ep", (0.3, 0.05, 0, 16000, 0.03)),
    ("ratio_1.5", "ep", (0.3, 1.5, 0, 16000, 0.03)),
    ("ratio_-0.5", "ep", (0.3, -0.5, 0, 16000, 0.03)),
    ("window_-1", "ep", (-1.0, 0.9, 0, 16000, 0.03)),
)


def load_results():
    return np.load(RESULTS_NPZ)


def load_endpoints():
    import json
    with open(ENDPOINTS_JSON) as fh:
        return json.load(fh)
