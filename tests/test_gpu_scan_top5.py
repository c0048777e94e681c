"""The selection of the matrix-core scan on the device: ssw_debug_scan_top5 lays caller-supplied
keys out the way the MFMA tiles deliver them (lane l of a wave: frame l % 32 of a column block,
the 16 rows 8 (r >> 2) + 4 (l / 32) + (r & 3) of each of the four row blocks) and runs the
production selection network, the swap of the wave's halves and the merge.  Expected values:
numpy's sort of the same labelled keys.  (The network itself is checked exhaustively on the CPU:
tests/test_top5_select_host.py.)"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _label(d):
    """label of density d = 32 rb + 8 q + 4 half + m: register (4 q + m) + 16 rb, bit 6 = half"""
    d = np.asarray(d)
    return (4 * ((d >> 3) & 3) + (d & 3)) + 16 * (d >> 5) + 64 * ((d >> 2) & 1)


def _density(half, pos):
    """density at position pos = r + 16 rb (0..63) of the list of a lane of the given half"""
    r, rb = pos & 15, pos >> 4
    return 32 * rb + 8 * (r >> 2) + 4 * half + (r & 3)


def _expected(keys):
    """the five largest labelled keys per frame: (densities, keys with the label bits cleared)"""
    lab = _label(np.arange(128)).astype(np.uint32)
    assert len(set(lab.tolist())) == 128 and lab.max() == 127
    bits = (np.ascontiguousarray(keys, np.float32).view(np.uint32) & np.uint32(0xffffff80)) | lab
    k = bits.view(np.float32)
    order = np.argsort(-k.astype(np.float64), axis=1, kind="stable")[:, :5]
    top = np.take_along_axis(bits, order, axis=1) & np.uint32(0xffffff80)
    return order.astype(np.int32), top.view(np.float32)


def _background(rng, n):
    """keys well below the placed ones, a different order in every frame, negative ones included"""
    return (-1000.0 - 16.0 * rng.permuted(np.tile(np.arange(128), (n, 1)), axis=1)).astype(np.float32)


def _reference_densities(rec, x):
    """rec float32 [128][32] exact records of one codebook x stream, x float32 [n][13]:
    d = det - sum_j (x_j - m_j)^2 v_j with one rounding per operation (src/ptm_mgau.c:63-68)."""
    mean, var, det = rec[:, 0:13], rec[:, 16:29], rec[:, 15]
    d = np.broadcast_to(det, (len(x), 128)).astype(np.float32).copy()
    for j in range(13):
        diff = x[:, None, j] - mean[None, :, j]
        sq = diff * diff
        d = d - sq * var[None, :, j]
    return d


# windows of nine positions that straddle the leftover 16th slot of a tile (13, 14, 15) and the
# end of the lane's list (61, 62, 63: they wrap into the first tile), for both halves of the wave
FIXED_WINDOWS = [(half, start) for start in (13, 14, 15, 61, 62, 63) for half in (0, 1)]


def _key_matrix(n):
    """One frame per case, kinds in rotation:
    0  the five largest within nine consecutive positions of ONE lane's list (a triple and its
       neighbours): first the FIXED_WINDOWS across the leftover 16th slot and the tile
       boundaries, then windows that move through the list
    1  the five largest all in the upper half's rows
    2  the five largest all in one row block (both halves)
    3  random keys of both signs, some differing in the label bits only
    plus a frame that is all -inf and a frame with one NaN in each wave."""
    rng = np.random.default_rng(20261018)
    keys = _background(rng, n)
    big = np.array([500.0, 400.0, 300.0, 200.0, 100.0], np.float32)
    for t in range(n):
        kind = t % 4
        if kind == 0:
            if (t >> 2) < len(FIXED_WINDOWS):
                half, start = FIXED_WINDOWS[t >> 2]
            else:
                half, start = (t >> 2) & 1, (5 * (t >> 2) + 13 * (t >> 3)) % 64
            pos = (start + rng.permutation(9)[:5]) % 64
            keys[t, _density(half, pos)] = big
        elif kind == 1:
            keys[t, _density(1, rng.permutation(64)[:5])] = big
        elif kind == 2:
            keys[t, 32 * int(rng.integers(0, 4)) + rng.permutation(32)[:5]] = big
        else:
            keys[t] = (rng.normal(0, 50, 128)).astype(np.float32)
            keys[t, rng.permutation(128)[:40]] = np.float32(37.25)   # equal but for the labels
    special = {}
    for w in range((n + 63) // 64):
        a, b = min(64 * w + 5, n - 2), min(64 * w + 34, n - 1)
        keys[a] = -np.inf
        keys[b, 77] = np.nan
        special[a] = special[b] = True
    return keys, np.array([t not in special for t in range(n)])


@pytest.mark.parametrize("n_frames", [64, 100])   # one wave; two, the second with a ragged tail
def test_selection_on_supplied_keys(gpu_en, n_frames):
    keys, ordinary = _key_matrix(n_frames)
    idx, top = gpu_en.debug_scan_top5(keys)
    assert idx.shape == (n_frames, 5) and top.shape == (n_frames, 5)
    # frames of -inf / NaN keys: the call returns and names densities (in the product such
    # frames always take the exact pass)
    assert (idx >= 0).all() and (idx < 128).all()
    want_idx, want_top = _expected(keys[ordinary])
    bad = np.flatnonzero((idx[ordinary] != want_idx).any(axis=1))
    assert len(bad) == 0, (len(bad), np.flatnonzero(ordinary)[bad][:8], idx[ordinary][bad[:2]],
                           want_idx[bad[:2]])
    assert np.array_equal(top[ordinary].view(np.uint32), want_top.view(np.uint32))


def test_selection_on_the_scans_own_keys(gpu_en):
    """Keys of the real scan (ssw_debug_scan_keys) on 128 frames of the reference's recording,
    for codebook x stream 0 (which leaves densities to the exact form: their keys are the exact
    values, as in the scan) and one other, back through the selection: equal to numpy's sort
    for every frame.  And against the product: the first four densities are the codewords the
    real scan wrote for every pair it proved.  An unproven pair is rewritten by the exact pass
    with the exact top 4, so every frame is decided: its codewords are the top 4 by keys, or
    they are four densities whose exact scores (the reference's arithmetic, truncated as
    dens2int truncates) are the four largest of the 128 and are the scores the scan wrote.
    The frames of the second kind are unproven pairs; tests/test_gpu_ptm.py allows this
    recording one pair in twenty of those, and the same share is allowed here."""
    g = gpu_en
    cep = np.load(os.path.join(ROOT, "tests", "golden", "goforward_mfcc.npy")).astype(np.float32)
    feats = np.ascontiguousarray(g.feat_batch(cep)[:128], np.float32)
    assert feats.shape == (128, 39)
    g.score_batch(feats)
    cw, sc = g.last_topn(len(feats))
    flagged, pairs = g.last_stats()
    n_cbf = g.n_cb * g.n_feat
    assert pairs == 128 * n_cbf
    rec = g.table("rec").reshape(n_cbf, 128, 32)
    d0 = g.table("scan_d0").reshape(n_cbf, 32)[:, 0]
    ex = g.table("scan_exact_mfma").reshape(n_cbf, 132)
    assert ex[0, 0] > 0, "codebook x stream 0 of en-us leaves densities to the exact form"
    differ = 0
    for cbf in (0, 3 * g.n_feat + 1):
        f = cbf % g.n_feat
        keys = g.debug_scan_keys(feats, cbf)
        ref = _reference_densities(rec[cbf], feats[:, f * 13:(f + 1) * 13])
        inert = ex[cbf, 1:1 + ex[cbf, 0]].astype(np.int64)
        if len(inert):
            keys[:, inert] = ref[:, inert] - np.float32(d0[cbf])
        idx, top = g.debug_scan_top5(keys)
        want_idx, want_top = _expected(keys)
        assert np.array_equal(idx, want_idx)
        assert np.array_equal(top.view(np.uint32), want_top.view(np.uint32))
        scan_cw = cw[:, cbf // g.n_feat, f, :].astype(np.int64)
        scan_sc = sc[:, cbf // g.n_feat, f, :].astype(np.int64)
        got4 = np.sort(idx[:, :4], axis=1)
        other = np.flatnonzero((got4 != np.sort(scan_cw, axis=1)).any(axis=1))
        # dens2int: truncation towards zero, INT_MIN below the int range
        assert np.isfinite(ref).all() and ref.max() < 2.0 ** 31
        r64 = ref.astype(np.float64)
        score = np.where(r64 >= -2.0 ** 31, np.trunc(r64), -2.0 ** 31).astype(np.int64)
        for t in other:
            best4 = np.sort(score[t])[-4:][::-1]
            assert np.array_equal(scan_sc[t], best4), (cbf, int(t), scan_sc[t], best4, idx[t])
            assert np.array_equal(score[t, scan_cw[t]], scan_sc[t]), (cbf, int(t), scan_cw[t])
            assert len(set(scan_cw[t].tolist())) == 4
        print("codebook x stream %d: %d of 128 frames carry the exact pass's codewords, not the "
              "top 4 by keys (%d of %d pairs of the batch unproven)"
              % (cbf, len(other), flagged, pairs))
        differ += len(other)
    assert differ <= flagged
    assert differ <= 2 * 128 // 20
