"""The two-level selection network, the fold from known positions and the merge by position of
the matrix-core scan on the device, through ssw_debug_scan_top5 (which lays caller-supplied keys
out the way the MFMA tiles deliver them and runs what the scan runs: ssw_top5_tile2,
ssw_top5_fold2, the swap of the wave's halves in registers, ssw_top5_merge).  The placements are
the ones the second level and the merge can get wrong: the five largest inside ONE tile of one
lane (the second-level triples span the tile), and split between the two halves of the wave.
Expected values: numpy's sort of the same labelled keys.  (The network itself is checked
exhaustively on the CPU: tests/test_top5_select2_host.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _label(d):
    """label of density d = 32 rb + 8 q + 4 half + m: register (4 q + m) + 16 rb, bit 6 = half"""
    d = np.asarray(d)
    return (4 * ((d >> 3) & 3) + (d & 3)) + 16 * (d >> 5) + 64 * ((d >> 2) & 1)


def _density(half, pos):
    """density at position pos = r + 16 rb (0..63) of the list of a lane of the given half"""
    pos = np.asarray(pos)
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


# Registers of a tile: level-1 triples (0 1 2) (3 4 5) (6 7 8) (9 10 11) (12 13 14), leftover 15;
# second level: the largest of the first three triples, and those of the last two with 15.
# Offsets from a rotating start, so that the five fall 5 + 0, 3 + 2, 2 + 2 + 1, ... across both
# levels' triples, onto and around the leftover key.
PATTERNS = [(0, 1, 2, 3, 4),       # a triple and most of its neighbour
            (0, 3, 6, 9, 12),      # one key per level-1 triple: five r1
            (0, 1, 3, 4, 9),       # 2 + 2 + 1
            (0, 3, 9, 12, 15),     # both second-level triples, the leftover key
            (0, 1, 2, 9, 10),      # 3 + 2
            (0, 6, 7, 8, 15)]


def _key_matrix(n):
    """One frame per case, kinds in rotation:
    0  the five largest inside the 16 rows of one row block of ONE half (one tile of one lane),
       the start rotating through all 16 positions, every pattern above and random ones
    1  the five largest split 3 / 2 and 4 / 1 between the halves, either way round
    2  random keys of both signs, 40 of them equal but for their labels, in turn among the
       others and above them all
    plus a frame that is all -inf and a frame with one NaN in each wave."""
    rng = np.random.default_rng(20261018)
    keys = (-1000.0 - 16.0 * rng.permuted(np.tile(np.arange(128), (n, 1)), axis=1)).astype(np.float32)
    big = np.array([500.0, 400.0, 300.0, 200.0, 100.0], np.float32)
    starts = set()
    for t in range(n):
        kind, j = t % 3, t // 3
        if kind == 0:
            start, half, rb = j % 16, (j + (j >> 4)) & 1, (j + (j >> 2)) & 3
            p = (j + j // 16) % (len(PATTERNS) + 1)
            pat = PATTERNS[p] if p < len(PATTERNS) else rng.permutation(16)[:5]
            pos = 16 * rb + (start + np.asarray(pat)) % 16
            assert len(set(pos.tolist())) == 5
            keys[t, _density(half, pos)] = rng.permutation(big)
            starts.add(start)
        elif kind == 1:
            n_lo = (3, 2, 4, 1)[j % 4]
            lo = _density(0, rng.permutation(64)[:n_lo])
            hi = _density(1, rng.permutation(64)[:5 - n_lo])
            keys[t, np.concatenate([lo, hi])] = rng.permutation(big)
        else:
            keys[t] = rng.normal(0, 50, 128).astype(np.float32)
            # equal but for the labels: among the other keys, or (odd j) above them all, so
            # that the labels alone decide the five
            keys[t, rng.permutation(128)[:40]] = np.float32(37.25 if j % 2 == 0 else 437.25)
    assert starts == set(range(16))
    special = {}
    for w in range((n + 63) // 64):
        a, b = min(64 * w + 5, n - 2), min(64 * w + 34, n - 1)
        keys[a] = -np.inf
        keys[b, 77] = np.nan
        special[a] = special[b] = True
    return keys, np.array([t not in special for t in range(n)])


@pytest.mark.parametrize("n_frames", [64, 100])   # one wave; two, the second with a ragged tail
def test_two_level_selection_and_merge_on_supplied_keys(gpu_en, n_frames):
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
