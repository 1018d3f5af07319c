"""The coverage model (tests/coverage_model.py) against its per-base form, on hand-made and random small cases."""
import random

import numpy as np
import pytest

import coverage_model as M

CASES = {
    "ends_on_a_bin_edge": ([(3, 20)], 10, 4),
    "starts_on_a_bin_edge": ([(10, 17)], 10, 4),
    "edge_to_edge": ([(10, 30)], 10, 4),
    "one_base": ([(9, 10), (10, 11), (0, 1), (39, 40)], 10, 4),
    "longer_than_all_bins": ([(2, 500)], 10, 4),
    "no_bins": ([(0, 5), (7, 30)], 10, 0),
    "overlapping_unsorted": ([(25, 60), (0, 30), (25, 26), (5, 45), (0, 30)], 7, 6),
    "empty_segments": ([(5, 5), (9, 3), (4, 6)], 4, 3),
    "wholly_outside": ([(40, 50), (100, 130)], 10, 4),
    "starts_in_last_bin": ([(39, 55)], 10, 4),
    "bin_size_one": ([(0, 3), (2, 9)], 1, 5),
    "nothing": ([], 10, 4),
}


def _same(segments, bin_size, n_bins):
    got, want = M.coverage(segments, bin_size, n_bins), M.coverage_naive(segments, bin_size, n_bins)
    for g, w, what in zip(got[:3], want[:3], ("bases", "starts", "ends")):
        assert g.dtype == np.int64 and np.array_equal(g, w), (what, g, w)
    assert got[3] == want[3]
    assert int(got[0].sum()) + got[3] == M.total_length(segments)
    return got


@pytest.mark.parametrize("name", sorted(CASES))
def test_hand_made(name):
    _same(*CASES[name])


def test_known_answer():
    bases, starts, ends, outside = _same([(3, 20), (25, 47)], 10, 4)
    assert bases.tolist() == [7, 10, 5, 10] and outside == 7
    assert starts.tolist() == [1, 0, 1, 0] and ends.tolist() == [0, 1, 0, 0]


@pytest.mark.parametrize("seed", range(40))
def test_random(seed):
    r = random.Random(seed)
    span = r.choice((30, 200, 700))
    segs = []
    for _ in range(r.randint(0, 30)):
        s = r.randint(0, span)
        segs.append((s, s + r.choice((0, 1, 2, 5, 40, span))))
    r.shuffle(segs)
    _same(segs, r.choice((1, 2, 7, 10, 64, span, 3 * span)), r.choice((0, 1, 2, 5, 40)))


def test_from_sample_layout():
    seg = np.array([(0, 5), (8, 12), (3, 4), (0, 30), (1, 2)], dtype=[("start", "<u4"), ("end", "<u4")])
    off = np.array([0, 2, 3, 4, 5])                    # two samples x two contigs
    bases, starts, ends, outside = M.from_sample(seg, off, 2, 10, [2, 1])
    assert bases.tolist() == [5 + 2 + 10, 2 + 10, 1 + 1] and outside.tolist() == [10, 0]
    assert starts.tolist() == [3, 0, 2] and ends.tolist() == [1, 1, 2]
