#!/usr/bin/env python3
"""Writes tests/golden/inputs_f32.npz and inputs_words.json: the reference library fed float32
audio (fe_process_float32, decoder_process_float32) and searching with words added to its loaded
dictionary (decoder_add_word, decoder_lookup_word), the truth that ssw_fe_batch_f32 and
ssw_dict_add_word are tested against.

It compiles tests/harness/inputs_driver.c against the reference library that build() makes in
oracle/_ref/ (oracle/reference.py) and runs it on the inputs tests/inputs_common.py makes.

inputs_f32.npz   "cep/<name>" per fixture of inputs_common.FE_FIXTURES: the float32 cepstra;
                 "align/<kind>/<rate>/<compallsen>": decoder_result_json at align_level 1 of
                 goforward as float32 aligned to "go forward ten meters", the line as uint8
inputs_words.json  per case of inputs_common.WORD_CASES and compallsen, "<case>/<yes|no>":
    adds       [[word, return value of decoder_add_word]] in the order of inputs_common.adds
    lookups    [[word, decoder_lookup_word or null]]
    fsg_search fsg_model_write of the searched grammar (after decoder_set_fsg), by line
    frames, hyp, score, segments, json1 (null without a hypothesis), errors
  The script asserts what the cases are there to pin: which alternate wins, that the word of
  unseen phone pairs is searched, and which adds the reference refuses.

    python tests/golden/make_inputs.py           # rewrite the fixtures
    python tests/golden/make_inputs.py --check   # rewrite nothing; exit 1 and name every
                                                 # fixture whose bytes would change
"""
import io
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import reference  # noqa: E402
from tests import fe_rates_common as R  # noqa: E402
from tests import inputs_common as I  # noqa: E402

MODELS = os.path.join(ROOT, "soundswallower_amd", "model")


def build_driver(tmp):
    exe = os.path.join(tmp, "inputs_driver")
    subprocess.run(["gcc", "-O1", "-std=gnu99", "-Wall", "-Werror", "-I" + reference.INCLUDE,
                    "-I" + reference.BUILD,
                    os.path.join(ROOT, "tests", "harness", "inputs_driver.c"), reference.LIBRARY,
                    "-lm", "-o", exe], check=True)
    return exe


def generate_f32(exe, tmp):
    arrays = {}
    raw = os.path.join(tmp, "pcm.f32")
    out = os.path.join(tmp, "cep.f32")
    for name, kind, rate, cfg, n in I.FE_FIXTURES:
        I.f32_pcm(kind, rate, n).astype("<f4").tofile(raw)
        r = subprocess.run([exe, "fe32", R.reference_json(cfg, rate), raw, out], check=True,
                           capture_output=True, text=True)
        cep = np.fromfile(out, dtype=np.float32).reshape(-1, 13)
        assert len(cep) == int(r.stdout), name
        arrays["cep/" + name] = cep
    for kind, rate in I.ALIGN_CASES:
        I.f32_pcm(kind, rate).astype("<f4").tofile(raw)
        for comp in I.CONFIGS:
            r = subprocess.run([exe, "align32", os.path.join(MODELS, "en-us"), str(rate), comp,
                                raw, I.ALIGN_TEXT], check=True, capture_output=True)
            arrays[I.align_key(kind, rate, comp)] = np.frombuffer(r.stdout, np.uint8).copy()
    return arrays


def run_words(exe, tmp, case, comp):
    name, model, recording, how, what = case
    adds = os.path.join(tmp, "adds.txt")
    with open(adds, "w", encoding="utf-8") as f:
        for w, p in I.adds(model):
            f.write(f"{w}\t{p}\n")
    if how == "fsg":
        arg = os.path.join(tmp, what[0] + ".fsg")
        with open(arg, "w", encoding="utf-8") as f:
            f.write(I.fsg_text(what))
    else:
        arg = what
    r = subprocess.run([exe, "words", os.path.join(MODELS, model), adds, comp,
                        os.path.join(I.GOLD, recording), arg], check=True, capture_output=True,
                       encoding="utf-8")
    rec = {"adds": [], "lookups": [], "fsg_search": [], "frames": None, "hyp": None, "score": None,
           "segments": [], "json1": None, "errors": []}
    for line in r.stdout.splitlines(keepends=True):
        tag, _, rest = line.partition(" ")
        rest_ = rest.rstrip("\n")
        if tag == "ADD":
            rv, _, w = rest_.partition(" ")
            rec["adds"].append([w, int(rv)])
        elif tag == "LOOKUP":
            w, _, ph = rest_.partition("\t")
            rec["lookups"].append([w, None if ph == "(NULL)" else ph])
        elif tag == "FSGX":
            rec["fsg_search"].append(rest_)
        elif tag == "FRAMES":
            rec["frames"] = int(rest)
        elif tag == "HYP":
            score, _, text = rest_.partition(" ")
            rec["hyp"], rec["score"] = text, int(score)
        elif tag == "SEG":
            t = rest_.split(" ", 5)
            rec["segments"].append([t[5]] + [int(x) for x in t[:5]])
        elif tag == "JSON1" and rest_ != "NOALIGN":
            rec["json1"] = rest
    for line in r.stderr.splitlines():
        rec["errors"].append(re.sub(r'^ERROR: "[^"]*", line \d+: ', "", line))
    return rec


def generate_words(exe, tmp):
    got = {I.word_key(c[0], comp): run_words(exe, tmp, c, comp)
           for c in I.WORD_CASES for comp in I.CONFIGS}
    # what the cases are there to pin
    for comp in I.CONFIGS:
        for c in I.WORD_CASES:
            rec = got[I.word_key(c[0], comp)]
            ok = [w for w, rv in rec["adds"] if rv >= 0]
            assert ok == [w for w, _ in I.added(c[1])], (c[0], rec["adds"])
            assert [w for w, _ in rec["adds"]] == [w for w, _ in I.adds(c[1])]
            # ("forward" was refused because it exists, with the pronunciation offered again)
            assert rec["lookups"] == [[w, " ".join(p.split()) if w in ok + ["forward"] else None]
                                      for w, p in I.adds(c[1])], (c[0], rec["lookups"])
        words = lambda k: [s[0] for s in got[I.word_key(k, comp)]["segments"]]
        assert "go" in words("plain") and not {"go(2)", "go(3)"} & set(words("plain"))   # they lose
        assert "tennn(2)" in words("alt_wins") and "tennn" not in words("alt_wins")
        assert "fourward" in words("respell")
        assert {"geee", "ohwe"} <= set(words("one_phone"))
        assert any(t.endswith(" zzpairs") for t in got[I.word_key("pairs_fsg", comp)]["fsg_search"])
        assert got[I.word_key("pairs_fsg", comp)]["json1"] is not None
        assert "mètrès" in words("fr")
    return got


def npz_bytes(arrays):
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    return buf.getvalue()


def differences(arrays, words):
    bad = []
    if not os.path.exists(I.F32_NPZ):
        bad.append(I.F32_NPZ)
    else:
        have = np.load(I.F32_NPZ)
        for k, v in arrays.items():
            if k not in have.files or have[k].dtype != v.dtype or have[k].tobytes() != v.tobytes():
                bad.append(k)
        bad += [k for k in have.files if k not in arrays]
    have = I.word_results() if os.path.exists(I.WORDS_JSON) else {}
    bad += [k for k in sorted(set(words) | set(have)) if have.get(k) != words.get(k)]
    return bad


def main():
    check = "--check" in sys.argv[1:]
    if not reference.available():
        sys.exit("no reference build in oracle/_ref/ (build() makes it from a SoundSwallower tree)")
    with tempfile.TemporaryDirectory() as tmp:
        exe = build_driver(tmp)
        arrays = generate_f32(exe, tmp)
        words = generate_words(exe, tmp)
    if check:
        bad = differences(arrays, words)
        for k in bad:
            print("differs:", k)
        sys.exit(1 if bad else 0)
    with open(I.F32_NPZ, "wb") as f:
        f.write(npz_bytes(arrays))
    with open(I.WORDS_JSON, "w", encoding="utf-8") as f:
        json.dump(words, f, indent=1, sort_keys=True, ensure_ascii=False)
        f.write("\n")
    print(f"{len(arrays)} arrays, {os.path.getsize(I.F32_NPZ)} bytes; {len(words)} word records, "
          f"{os.path.getsize(I.WORDS_JSON)} bytes")


if __name__ == "__main__":
    main()
