"""Voice activity detection and endpointing, host side (no GPU): ssw_vad_batch_host -- built from
the arithmetic source the kernel is built from -- against every decision the reference's
vad_classify made (tests/golden/vad_results.npz), ssw_endpoints_from_decisions against every
segment its endpointer cut, with the times as exact doubles (vad_endpoints.json), the refusals in
the reference's words, the accessors, a stream fed in two pieces through `state`, and (where
build() made the reference library) that the committed fixtures are what the reference makes."""
import os
import subprocess
import sys

import numpy as np
import pytest

import soundswallower_amd as ssw
from oracle import reference
from soundswallower_amd import _lib
from tests import vad_common as V
from tests.conftest import ROOT


@pytest.fixture(scope="module", autouse=True)
def built():
    _lib.build()


@pytest.fixture(scope="module")
def recorded():
    return V.load_results()


@pytest.fixture(scope="module")
def endpoints():
    return V.load_endpoints()


def _configs(cases):
    """the cases grouped by the detector they need: {(mode, rate, frame_length): [case, ...]}"""
    groups = {}
    for c in cases:
        groups.setdefault((c[2], c[3], c[4]), []).append(c)
    return groups


def test_fixtures_hold_speech_and_silence(recorded):
    """the condition make_vad.py asserts when recording, on the committed bytes: between 10 % and
    90 % of every speech fixture's frames are speech, and each is at least 400 frames long"""
    for (case, *_rest) in V.SPEECH_CASES:
        dec = recorded["dec/" + case]
        assert len(dec) >= 400, case
        assert 0.10 <= float((dec != 0).mean()) <= 0.90, case


@pytest.mark.parametrize("config", sorted(_configs(V.VAD_CASES)), ids=lambda c: "m%d_r%d_f%g" % c)
def test_host_decisions_equal_the_reference(config, recorded):
    mode, rate, fl = config
    vad = ssw.Vad(mode, rate, fl)
    cases = _configs(V.VAD_CASES)[config]
    pcm = [V.stream(c[1], rate) for c in cases]
    off = np.concatenate([[0], np.cumsum([len(p) for p in pcm])]).astype(np.int64)
    dec, frame_off = vad.classify_batch_host(np.concatenate(pcm), off)
    for i, c in enumerate(cases):
        want = recorded["dec/" + c[0]]
        got = dec[frame_off[i]:frame_off[i + 1]]
        assert got.shape == want.shape and np.array_equal(got, want), c[0]


@pytest.mark.parametrize("case", V.EP_CASES, ids=lambda c: c[0])
def test_host_segments_equal_the_reference(case, endpoints):
    name, _, mode, rate, fl, window, ratio, _ = case
    vad = ssw.Vad(mode, rate, fl)
    pcm = V.ep_input(case)
    dec, _ = vad.classify_batch_host(pcm, [0, len(pcm)])
    segs = vad.endpoints_from_decisions(dec, len(pcm) % vad.frame_size, window, ratio)
    want = endpoints["segments"][name]
    assert len(want) > 0, name
    got = [[int(s["first_sample"]), int(s["n_samples"]), float(s["speech_start"]),
            float(s["speech_end"])] for s in segs]
    # float() of 17 significant digits is the double the reference printed: equality is exact
    assert got == [[a, b, float(c), float(d)] for (a, b, c, d) in want], name


def test_trailing_samples_reach_the_last_segment(endpoints):
    """the streams cut inside an utterance: end_stream hands the tail back, so the last segment of
    the stream that leaves size - 1 samples is that much longer than the one that leaves none"""
    for tag in ("w3", "w5"):
        n0 = endpoints["segments"][f"goforward_r16000_m0_f30_{tag}_t0"][-1][1]
        n1 = endpoints["segments"][f"goforward_r16000_m0_f30_{tag}_t1"][-1][1]
        n479 = endpoints["segments"][f"goforward_r16000_m0_f30_{tag}_tsize-1"][-1][1]
        assert (n1 - n0, n479 - n0) == (1, 479)


@pytest.mark.parametrize("case,kind,args", V.REFUSALS, ids=[r[0] for r in V.REFUSALS])
def test_refusals_carry_the_reference_text(case, kind, args, endpoints):
    words = endpoints["refusals"][case]
    with pytest.raises(ssw.SswError) as e:
        if kind == "vad":
            ssw.Vad(*args)
        else:
            window, ratio, mode, rate, fl = args
            ssw.Vad(mode, rate, fl).endpoints_from_decisions(np.zeros(4, np.int8), 0, window, ratio)
    assert str(e.value).endswith(": " + words), (str(e.value), words)


@pytest.mark.parametrize("rate,fl,size,closest", [
    (16000, 0.03, 480, 16000), (0, 0, 480, 16000), (8000, 0.01, 80, 8000), (32000, 0.02, 640, 32000),
    (48000, 0.03, 1440, 48000), (44100, 0.03, 1440, 48000), (22050, 0.02, 320, 16000),
    (11025, 0.01, 80, 8000)])
def test_accessors_return_what_the_reference_macros_return(rate, fl, size, closest):
    vad = ssw.Vad(0, rate, fl)
    caller = rate or 16000
    assert (vad.frame_size, vad.closest_rate, vad.sample_rate) == (size, closest, caller)
    assert vad.frame_length == size / caller          # vad_frame_length: size / the caller's rate
    assert [vad.frame_count(n) for n in (0, size - 1, size, 2 * size + 1)] == [0, 0, 1, 2]


@pytest.mark.parametrize("rate", (8000, 16000, 32000, 48000))
def test_a_stream_in_two_pieces_is_the_stream_whole(rate):
    vad = ssw.Vad(1, rate, 0.03)
    pcm = V.stream("goforward", rate)
    n = len(pcm) // vad.frame_size
    whole, _, feat = vad.classify_batch_host(pcm, [0, len(pcm)], features=True)
    state = np.zeros(1, ssw.VAD_STATE_DTYPE)            # not set up: the call starts afresh
    cut = (n // 3) * vad.frame_size
    a, _, fa = vad.classify_batch_host(pcm[:cut], [0, cut], state=state, features=True)
    assert int(state["initialised"][0]) == 42 and int(state["frame_counter"][0]) > 0
    b, _, fb = vad.classify_batch_host(pcm[cut:], [0, len(pcm) - cut], state=state, features=True)
    assert np.array_equal(np.concatenate([a, b]), whole)
    assert np.array_equal(np.concatenate([fa, fb]), feat)
    fresh = vad.new_states(1)
    assert int(fresh["initialised"][0]) == 42 and int(fresh["mean_value"][0][0]) == 1600
    c, _ = vad.classify_batch_host(pcm[:cut], [0, cut], state=fresh)
    assert np.array_equal(c, a) and fresh.tobytes() != vad.new_states(1).tobytes()


def test_float_audio_is_refused_with_a_message():
    vad = ssw.Vad()
    for dt in (np.float32, np.float64, np.float16):
        with pytest.raises(ssw.SswError, match="int16 samples, so scale float audio yourself"):
            vad.classify_batch_host(np.zeros(960, dt), [0, 960])


def test_empty_and_short_streams():
    vad = ssw.Vad()
    pcm = V.stream("goforward", 16000)[:1000]
    dec, frame_off = vad.classify_batch_host(pcm, [0, 0, 479, 1000])
    assert frame_off.tolist() == [0, 0, 0, 1] and len(dec) == 1
    assert vad.endpoints_from_decisions(np.zeros(0, np.int8), 0).shape == (0,)


@pytest.mark.skipif(not reference.available(), reason="no reference build in oracle/_ref/")
def test_committed_fixtures_are_what_the_reference_makes():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_vad.py"),
                        "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_streams_per_workgroup_takes_its_five_values():
    vad = ssw.Vad()
    for k in (8, 16, 32, 64, 0):
        vad.set_streams_per_workgroup(k)
    with pytest.raises(ssw.SswError, match="0, 8, 16, 32 or 64"):
        vad.set_streams_per_workgroup(7)
