"""What tests/golden/make_inputs.py records and the tests of float32 audio and of words added at
run time replay.

Float audio is not committed.  It is made here from goforward.raw (and its integer resampling,
fe_rates_common.resample) with IEEE float32 +, x and / on integer-valued arrays only, so its
bytes are the same on every machine: no sin, no random numbers.  1.0 stands for 32768, the scale
of the reference's fe_process_float32.

inputs_f32.npz holds "cep/<name>" per fixture of FE_FIXTURES (fe_process_float32 + fe_end) and
"align/<kind>/<rate>/<compallsen>" (decoder_process_float32, decoder_result_json at level 1, as
bytes); inputs_words.json holds one record per case of WORD_CASES and configuration."""
import json
import os

import numpy as np

from tests import fe_rates_common as R

GOLD = R.GOLD
F32_NPZ = os.path.join(GOLD, "inputs_f32.npz")
WORDS_JSON = os.path.join(GOLD, "inputs_words.json")

_F = np.float32


def _ints(x):
    return np.asarray(x, np.int64).astype(np.float32)      # |x| <= 32768: exact


# kind -> int16 samples -> float32 samples
KINDS = {
    # exactly the int16 audio: the quotient by a power of two is exact
    "exact": lambda x: _ints(x) / _F(32768),
    # fractional sample values: x 0.37f / 32768 + 1 / 65536 (0.37f as 37 / 100 in float32)
    "frac": lambda x: _ints(x) * (_F(37) / _F(100)) / _F(32768) + _F(1) / _F(65536),
    # three times the recording (its peak is near 0.21, so this one stays inside +-1) ...
    "beyond": lambda x: _ints(x) * _F(3) / _F(32768),
    # ... and sixteen times: well beyond +-1, which the reference does not clip
    "loud": lambda x: _ints(x) * _F(16) / _F(32768),
    # tiny: x / 2^40
    "tiny": lambda x: _ints(x) / _F(2 ** 40),
    "zero": lambda x: np.zeros(len(x), np.float32),
}


def int_pcm(rate, n=None):
    """goforward at `rate` Hz as int16, its first n samples when n is given"""
    y = R.goforward() if rate == 16000 else R.resample(R.goforward(), rate)
    return y if n is None else y[:n].copy()


def f32_pcm(kind, rate, n=None):
    out = KINDS[kind](int_pcm(rate, n))
    assert out.dtype == np.float32
    return out


def edge_lengths(rate):
    shift, size = R.framing(rate)
    return (1, size - 1, size, size + 1, size + shift - 1, size + shift, size + shift + 1)


def _fe_fixtures():
    """(name, kind, rate, front-end overrides, samples)"""
    fx = []
    for kind in KINDS:                       # 1 s at 16 kHz: dct and legacy, remove_noise on and off
        for transform in ("dct", "legacy"):
            for noise in (True, False):
                fx.append((f"{kind}_{transform}_n{int(noise)}", kind, 16000,
                           {"transform": transform, "remove_noise": noise}, 16000))
    for kind in KINDS:                       # 1 s at 44.1 kHz, the model's settings
        fx.append((f"{kind}_44100", kind, 44100, {}, 44100))
    for rate in (16000, 44100):              # the lengths around one window and one shift
        for n in edge_lengths(rate):
            fx.append((f"edge{rate}_{n}", "frac", rate, {}, n))
    return fx


FE_FIXTURES = _fe_fixtures()

# decoder_process_float32 of the whole recording, "go forward ten meters": (kind, rate)
ALIGN_CASES = (("exact", 16000), ("frac", 16000), ("beyond", 16000), ("loud", 16000),
               ("frac", 44100))
ALIGN_TEXT = R.ALIGN_TEXT
CONFIGS = ("yes", "no")                      # compallsen


def align_key(kind, rate, comp):
    return f"align/{kind}/{rate}/{comp}"


# ---------------------------------------------------------------------------------------------
# words added at run time
# ---------------------------------------------------------------------------------------------
def dictionary(model):
    """[(word, [phones])] of a shipped model's dict.txt, in file order"""
    out = []
    with open(os.path.join(R.ROOT, "soundswallower_amd", "model", model, "dict.txt"),
              encoding="utf-8") as f:
        for line in f:
            t = line.split()
            if len(t) > 1 and not line.startswith(("##", ";;")):
                out.append((t[0], t[1:]))
    return out


def unseen_pair_word(model="en-us"):
    """A pronunciation whose first two and last two phones begin and end no word of the
    dictionary: the first such pairs in the order of the dictionary's own phone list, around the
    pronunciation of "ten" (so the word can be told from noise).  The reference's
    dict2pid_add_word has to extend its cross-word tables for such a word."""
    prons = [p for _, p in dictionary(model) if len(p) >= 2]
    phones = sorted({ph for p in prons for ph in p})
    first = {(p[0], p[1]) for p in prons}
    last = {(p[-2], p[-1]) for p in prons}
    head = next((a, b) for a in phones for b in phones if (a, b) not in first)
    tail = next((a, b) for a in reversed(phones) for b in reversed(phones) if (a, b) not in last)
    return list(head) + ["T", "EH", "N"] + list(tail)


EN_ADDS = (
    ("fourward", "F AO R W ER D"),           # a new spelling of an existing pronunciation
    ("tennn", "T UW"),                        # a wrong base pronunciation ...
    ("tennn(2)", "T EH N"),                   # ... whose alternate wins the first pass
    ("go(2)", "G UW"),                       # alternates that lose it: two, so that the
    ("go(3)", "G AO"),                       # order of a word's added alternates is pinned
    ("geee", "G"), ("ohwe", "OW"),            # one-phone words
    ("zzpairs", None),                       # unseen_pair_word(), filled in below
    # refusals, recorded as the reference returns them
    ("forward", "F AO R W ER D"),            # exists
    ("nophone", "F XX"),                     # unknown phone
    ("nobase(2)", "T EH N"),                 # no base word
)
FR_ADDS = (("mètrès", "mm ai tt rr"),        # non-ASCII letters
           ("dîx(2)", "dd ii ss"),           # no base word
           ("avance(7)", "aa vv an ss ee"))     # one more alternate of avance


def adds(model):
    if model == "fr-fr":
        return list(FR_ADDS)
    return [(w, p if p is not None else " ".join(unseen_pair_word())) for w, p in EN_ADDS]


def added(model):
    """the adds the reference accepts: all but the three refusals of en-us, the one of fr-fr"""
    return [(w, p) for w, p in adds(model) if w not in ("forward", "nophone", "nobase(2)", "dîx(2)")]


# (case, model, recording, "text" | "fsg", text or (name, n_states, start, final, transitions))
WORD_CASES = (
    ("plain", "en-us", "goforward.raw", "text", "go forward ten meters"),      # no added word
    ("respell", "en-us", "goforward.raw", "text", "go fourward ten meters"),
    ("alt_wins", "en-us", "goforward.raw", "text", "go forward tennn meters"),
    ("one_phone", "en-us", "goforward.raw", "text", "geee ohwe forward ten meters"),
    ("pairs_text", "en-us", "goforward.raw", "text", "go forward zzpairs meters"),
    ("pairs_fsg", "en-us", "goforward.raw", "fsg",
     ("pairs", 5, 0, 4, ((0, 1, 1.0, "go"), (1, 2, 0.5, "forward"), (1, 2, 0.5, "zzpairs"),
                         (1, 2, 0.5, "fourward"), (2, 3, 0.5, "ten"), (2, 3, 0.5, "tennn"),
                         (3, 4, 1.0, "meters")))),
    ("fr", "fr-fr", "goforward_fr.raw", "text", "avance de dix mètrès"),
)


def fsg_text(spec):
    name, n, start, final, trans = spec
    lines = [f"FSG_BEGIN {name}", f"NUM_STATES {n}", f"START_STATE {start}", f"FINAL_STATE {final}"]
    lines += [f"TRANSITION {a} {b} {p} {w}" for a, b, p, w in trans]
    return "\n".join(lines + ["FSG_END"]) + "\n"


def word_key(case, comp):
    return f"{case}/{comp}"


def word_results():
    with open(WORDS_JSON, encoding="utf-8") as f:
        return json.load(f)


def recording(name):
    return np.fromfile(os.path.join(GOLD, name), dtype="<i2")
