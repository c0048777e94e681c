"""Voice activity detection and endpointing on the GPU: ssw_vad_batch against every decision the
reference's vad_classify made (tests/golden/vad_results.npz), ragged batches against the host
path (decisions, features and final state, stream for stream), the 48 kHz repeated block, a stream
split over two calls through `state`, ssw_endpoint_batch against the reference's segments
(vad_endpoints.json), and endpoint_audio_batch(...).utterances() into recognize_audio_batch.

All of it is integer arithmetic: everything is compared for equality."""
import os

import numpy as np
import pytest

import soundswallower_amd as ssw
from tests import jsgf_common as J
from tests import vad_common as V
from tests.conftest import MODEL_ROOT

pytestmark = pytest.mark.gpu


def _configs(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c[2], c[3], c[4]), []).append(c)
    return groups


def _offsets(pcms):
    return np.concatenate([[0], np.cumsum([len(p) for p in pcms])]).astype(np.int64)


@pytest.fixture(scope="module")
def recorded():
    return V.load_results()


@pytest.fixture(scope="module")
def endpoints():
    return V.load_endpoints()


@pytest.mark.parametrize("rate", V.RATES)
def test_recorded_decisions(rate, recorded):
    """every recorded fixture of the rate, the fixtures that share a detector as one batch"""
    n = 0
    for (mode, r, fl), cases in sorted(_configs(V.VAD_CASES).items()):
        if r != rate:
            continue
        vad = ssw.Vad(mode, rate, fl)
        pcms = [V.stream(c[1], rate) for c in cases]
        dec, frame_off = vad.classify_batch(np.concatenate(pcms), _offsets(pcms))
        for i, c in enumerate(cases):
            want = recorded["dec/" + c[0]]
            got = dec[frame_off[i]:frame_off[i + 1]]
            assert got.shape == want.shape and np.array_equal(got, want), c[0]
            n += 1
    assert n == sum(1 for c in V.VAD_CASES if c[3] == rate)


def _ragged(n_streams, size, rate, seed):
    """n_streams pieces of the speech fixture, their lengths drawn from the set the kernel's paths
    turn on -- nothing, less than a frame, 1, 2, 101, 103 and 400 frames, each with a few samples
    over -- mixed within the batch; every length appears when there are at least 7 streams"""
    rng = np.random.default_rng(seed)
    src = np.concatenate([V.stream("goforward", rate), V.stream("goforward_fr", rate)])
    lengths = [0, size - 1, size, 2 * size, 101 * size, 103 * size, 400 * size]
    pcms = []
    for u in range(n_streams):
        n = lengths[u % 7] if n_streams >= 7 else lengths[6]
        n += int(rng.integers(0, 3)) if n >= size else 0
        start = int(rng.integers(0, len(src) - n + 1))
        pcms.append(src[start:start + n])
    order = rng.permutation(n_streams)
    return [pcms[i] for i in order]


@pytest.mark.parametrize("n_streams,config,spw", [
    (1, (0, 16000, 0.03), None), (63, (0, 16000, 0.03), None), (64, (0, 16000, 0.03), "64"),
    (65, (0, 16000, 0.03), "64"), (65, (3, 16000, 0.03), None), (130, (0, 16000, 0.03), None),
    (130, (1, 16000, 0.03), "64"), (65, (2, 8000, 0.01), "64"), (65, (1, 32000, 0.02), "32"),
    (65, (0, 48000, 0.03), "64"), (130, (3, 48000, 0.02), "16")],
    ids=lambda x: None if x is None else str(x).replace(" ", ""))
def test_ragged_batches_against_the_host_path(n_streams, config, spw):
    """decisions, the parity view of the features and the final state of every stream equal the
    host path's; spw: the streams a workgroup takes, forced (the 64 a full wave takes included)"""
    mode, rate, fl = config
    vad = ssw.Vad(mode, rate, fl)
    if spw is not None:
        vad.set_streams_per_workgroup(int(spw))
    pcms = _ragged(n_streams, vad.frame_size, rate, 1000 + n_streams)
    pcm, off = np.concatenate(pcms), _offsets(pcms)
    state_h = np.zeros(n_streams, ssw.VAD_STATE_DTYPE)
    state_d = np.zeros(n_streams, ssw.VAD_STATE_DTYPE)
    want, fo_h, feat_h = vad.classify_batch_host(pcm, off, state=state_h, features=True)
    got, fo_d = vad.classify_batch(pcm, off, state=state_d)
    feat_d = vad.debug_features(len(got))
    assert np.array_equal(fo_d, fo_h) and fo_h[-1] > 0
    for u in range(n_streams):
        a, b = fo_h[u], fo_h[u + 1]
        assert np.array_equal(got[a:b], want[a:b]), f"decisions of stream {u} ({b - a} frames)"
        assert np.array_equal(feat_d[a:b], feat_h[a:b]), f"features of stream {u}"
        assert state_d[u:u + 1].tobytes() == state_h[u:u + 1].tobytes(), f"state of stream {u}"
    assert 0 < int(want.sum()) < len(want)
    # ... and without `state`: every stream afresh, the same decisions
    again, _ = vad.classify_batch(pcm, off)
    assert np.array_equal(again, want)


def test_48khz_resamples_the_first_10ms_of_each_frame_again(recorded):
    """WebRtcVad_CalcVad48khz hands the resampler the frame's start on every 10 ms iteration: at
    30 ms the second and third 10 ms of a frame are never read.  The decisions are the recorded
    ones, and they do not change when those two blocks are zeroed."""
    vad = ssw.Vad(0, 48000, 0.03)
    pcm = V.stream("goforward", 48000)
    n = len(pcm) // 1440
    frames = pcm[:n * 1440].reshape(n, 1440)
    assert np.any(frames[:, 480:960] != frames[:, :480]) and np.any(frames[:, 960:] != frames[:, :480])
    zeroed = frames.copy()
    zeroed[:, 480:] = 0
    both = np.concatenate([pcm, zeroed.reshape(-1)])
    dec, fo = vad.classify_batch(both, [0, len(pcm), len(both)])
    want = recorded["dec/goforward_r48000_m0_f30"]
    assert np.array_equal(dec[fo[0]:fo[1]], want)
    assert np.array_equal(dec[fo[1]:fo[2]], want)


@pytest.mark.parametrize("rate,fl", [(16000, 0.03), (48000, 0.02), (32000, 0.01), (8000, 0.03)])
def test_state_round_trip(rate, fl, recorded):
    """a stream split at a frame boundary over two calls, beside one that is given whole"""
    vad = ssw.Vad(3, rate, fl)
    a, b = V.stream("goforward", rate), V.stream("goforward_fr", rate)
    cut = (len(a) // vad.frame_size // 3) * vad.frame_size
    state = np.zeros(2, ssw.VAD_STATE_DTYPE)
    first, fo1 = vad.classify_batch(np.concatenate([a[:cut], b]), [0, cut, cut + len(b)], state=state)
    second, fo2 = vad.classify_batch(a[cut:], [0, len(a) - cut, len(a) - cut], state=state)
    ms = int(round(fl * 1000))
    assert np.array_equal(np.concatenate([first[:fo1[1]], second]),
                          recorded[f"dec/goforward_r{rate}_m3_f{ms}"])
    assert np.array_equal(first[fo1[1]:], recorded[f"dec/goforward_fr_r{rate}_m3_f{ms}"])
    assert fo2.tolist() == [0, len(second), len(second)]


def _ep_groups():
    groups = {}
    for c in V.EP_CASES:
        groups.setdefault(c[2:7], []).append(c)
    return groups


@pytest.mark.parametrize("key", sorted(_ep_groups()), ids=lambda k: "m%d_r%d_f%g_w%g_%g" % k)
def test_endpoint_batch_equals_the_recorded_segments(key, endpoints):
    mode, rate, fl, window, ratio = key
    cases = _ep_groups()[key]
    pcms = [V.ep_input(c) for c in cases]
    ep = ssw.endpoint_audio_batch(np.concatenate(pcms), _offsets(pcms), samprate=rate, mode=mode,
                                  window=window, ratio=ratio, frame_length=fl)
    for u, c in enumerate(cases):
        want = endpoints["segments"][c[0]]
        got = [[int(s["first_sample"]), int(s["n_samples"]), float(s["speech_start"]),
                float(s["speech_end"])] for s in ep.segments(u)]
        assert got == [[a, b, float(x), float(y)] for (a, b, x, y) in want], c[0]


def test_refusals_on_the_device_entry_points(endpoints):
    pcm = V.stream("goforward", 16000)
    with pytest.raises(ssw.SswError, match="end-pointing stupid or impossible"):
        ssw.endpoint_audio_batch(pcm, [0, len(pcm)], ratio=0.999)
    with pytest.raises(ssw.SswError, match="int16 samples, so scale float audio yourself"):
        ssw.endpoint_audio_batch(pcm.astype(np.float32), [0, len(pcm)])
    import torch
    with pytest.raises(ssw.SswError, match="int16 samples, so scale float audio yourself"):
        ssw.Vad().classify_batch(torch.zeros(960, dtype=torch.float32, device="cuda"), [0, 960])


def test_utterances_feed_recognition_like_ranges_cut_by_hand(gpu_en, endpoints):
    """plumbing only: the gathered utterances give, segment for segment, what recognising the same
    sample ranges -- cut by hand from the RECORDED segments -- gives; no claim about the words"""
    import torch
    names = ("goforward_r16000_m0_f30_w3", "goforward_r16000_m0_f30_w3_tsize-1")
    cases = [next(c for c in V.EP_CASES if c[0] == n) for n in names]
    pcms = [V.ep_input(c) for c in cases]
    off = _offsets(pcms)
    d_pcm = torch.from_numpy(np.concatenate(pcms)).to("cuda")     # a device tensor in
    ep = ssw.endpoint_audio_batch(d_pcm, off)
    u_pcm, u_off, stream_of, start = ep.utterances()
    want = [(u, s) for u, n in enumerate(names) for s in endpoints["segments"][n]]
    assert len(want) >= 4 and stream_of.tolist() == [u for u, _ in want]
    assert start.tolist() == [float(s[2]) for _, s in want]
    assert np.diff(u_off).tolist() == [s[1] for _, s in want]
    by_hand = [pcms[u][s[0]:s[0] + s[1]] for u, s in want]
    assert np.array_equal(u_pcm.cpu().numpy(), np.concatenate(by_hand))
    d = os.path.join(MODEL_ROOT, "en-us")
    lex = ssw.Lexicon(gpu_en, os.path.join(d, "dict.txt"), os.path.join(d, "noisedict.txt"))
    plan = lex.grammar_plan([ssw.Fsg.from_jsgf(gpu_en, lex, path=J.gram_path("turtle"))])
    got = ssw.recognize_audio_batch(gpu_en, lex, u_pcm, u_off, plan)
    ref = ssw.recognize_audio_batch(gpu_en, lex, np.concatenate(by_hand), _offsets(by_hand), plan)
    for k in range(len(want)):
        assert (got.status(k), got.hyp(k), got.score(k), [list(s) for s in got.segments(k)]) == \
            (ref.status(k), ref.hyp(k), ref.score(k), [list(s) for s in ref.segments(k)]), k
