"""CPU: `bench.py --dump-outputs DIR` -- what the last timed step computed, written so that two
builds can be compared output for output: float32, exact for the int16 scores, at most 64 MB,
and the same seeded sample of frames on every run."""
import os

import numpy as np

import bench


def _scores(n, n_sen, seed):
    return np.random.default_rng(seed).integers(-32768, 32767, (n, n_sen), dtype=np.int16)


def test_a_small_step_is_written_whole(tmp_path):
    s = _scores(512, 700, 1)
    bench.dump_outputs(str(tmp_path), s)
    got = np.load(tmp_path / "senone_scores.npy")
    rows = np.load(tmp_path / "senone_scores_frames.npy")
    assert got.dtype == np.float32 and rows.dtype == np.float64
    assert np.array_equal(got, s.astype(np.float32))
    assert np.array_equal(rows, np.arange(512))


def test_the_bench_step_is_sampled_under_the_cap_and_reproducibly(tmp_path):
    s = _scores(4096, 5126, 2)                      # the en-us step: 80 MB as float32
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), s)
    bench.dump_outputs(str(b), s)
    total = sum(os.path.getsize(os.path.join(a, f)) for f in os.listdir(a))
    assert total <= 64 * 10**6
    got = np.load(a / "senone_scores.npy")
    rows = np.load(a / "senone_scores_frames.npy").astype(np.int64)
    assert got.shape == (len(rows), 5126) and len(rows) > 2048
    assert np.all(np.diff(rows) > 0) and rows[-1] < 4096
    assert np.array_equal(got, s[rows].astype(np.float32))
    assert np.array_equal(rows, np.load(b / "senone_scores_frames.npy"))
    assert np.array_equal(got, np.load(b / "senone_scores.npy"))
