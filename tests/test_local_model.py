"""CPU: the numpy model of the per-bin overlaps (tests/local_model.py) against a loop over the bases, and its five words against
plain Python on the rows of sample values."""
import random

import numpy as np
import pytest

import local_model as M

BIN_SIZES = (1, 3, 7, 50)


@pytest.mark.parametrize("bin_size", BIN_SIZES)
def test_values_equal_the_loop_over_the_bases(bin_size):
    r = random.Random(bin_size)
    seen_beyond = seen_whole = False
    for _ in range(150):
        L = M.random_normalized(r, r.choice([0, 1, 3, 12]), 200, max_len=r.choice([1, 5, 60]))
        A = M.random_normalized(r, r.choice([0, 1, 4, 15]), 200, max_len=r.choice([1, 5, 60]))
        assert M.is_normalized(L) and M.is_normalized(A)
        top = max([e for _, e in L + A] + [0])
        for n_bins in {0, 1, (top + bin_size - 1) // bin_size, max(0, top // bin_size - 2)}:
            got = M.values(L, A, bin_size, n_bins)
            want = M.brute_values(L, A, bin_size, n_bins)
            assert got.dtype == np.int64 and got.tolist() == want, (L, A, bin_size, n_bins)
            assert all(0 <= v <= bin_size for v in want)
            seen_beyond |= sum(want) < sum(M.brute_values(L, A, bin_size, 200))
            seen_whole |= bin_size > 1 and bin_size in want
    assert seen_beyond and (seen_whole or bin_size in (1, 50))


def test_hand_values():
    # a piece ending on a bin edge, bookended intervals on both sides, a one-base overlap
    assert M.values([(0, 10), (10, 20)], [(5, 10), (10, 12), (19, 40)], 10, 3).tolist() == [5, 3, 0]
    assert M.values([(0, 100)], [(7, 8)], 1, 10).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 0, 0]
    assert M.values([(0, 100)], [(0, 100)], 7, 3).tolist() == [7, 7, 7]
    assert M.values([], [(0, 100)], 7, 3).tolist() == [0, 0, 0] and M.values([(1, 2)], [(1, 2)], 7, 0).tolist() == []
    top = 2 ** 32 - 1
    assert M.values([(5, top)], [(2 ** 31 - 1, 2 ** 31 + 1), (top - 1, top)], 2 ** 31, 2).tolist() == [1, 2]


def test_words():
    r = random.Random(3)
    v = np.array([[[r.choice([0, 0, 0, 1, 5, 9]) for _ in range(6)] for _ in range(2)] for _ in range(11)], dtype=np.int64)
    obs = np.array([[0, 1, 5, 9, 3, 100], [9, 0, 0, 5, 1, 2]], dtype=np.int64)
    w = M.words(v, obs)
    for t in range(2):
        for b in range(6):
            row, o = v[:, t, b].tolist(), int(obs[t, b])
            assert w[t, b].tolist() == [sum(1 for x in row if x > 0), sum(row), sum(x * x for x in row), sum(1 for x in row if x < o),
                                        sum(1 for x in row if x == o)]
    # additive over the samples
    assert np.array_equal(M.words(v[:4], obs) + M.words(v[4:], obs), w)
    big = np.full((3, 1, 1), 2 ** 31, dtype=np.int64)
    assert M.words(big, np.array([[2 ** 31]])).tolist() == [[[3, 3 * 2 ** 31, 3 * 2 ** 62 - 2 ** 64, 0, 3]]]     # (sumsq is unsigned: below 2^64)


def test_from_sample_layout():
    seg = np.zeros(3, dtype=[("start", "<u4"), ("end", "<u4")])
    seg["start"], seg["end"] = [0, 5, 2], [4, 9, 3]
    off = np.array([0, 2, 2, 2, 3], dtype=np.int64)          # sample 0: contig 0 has two segments; sample 1: contig 1 has one
    tracks = [[[(0, 100)], [(0, 100)]]]
    assert M.from_sample(seg, off, 2, tracks, 4, [3, 1]).tolist() == [[[4, 3, 1, 0]], [[0, 0, 0, 1]]]
