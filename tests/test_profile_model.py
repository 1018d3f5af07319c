"""The model of the profile around anchors (tests/profile_model.py) against the definition base by base, the worked example of
include/gat_mi355.h, the stated bounds, and the arithmetic of the five words: additive over a split of the samples, and
k_null_finish's count of the samples with v == 0.  No GPU."""
import random

import numpy as np

import profile_model as M


def test_worked_example():
    seg = [(85, 112)]
    assert M.values(seg, [(100, +1)], 10, 2).tolist() == [5, 10, 10, 2]
    assert M.values(seg, [(100, -1)], 10, 2).tolist() == [1, 10, 10, 6]
    assert M.values(seg, [(100, +1)], 10, 2, M.MIDPOINTS).tolist() == [0, 1, 0, 0]
    assert M.values(seg, [(100, -1)], 10, 2, M.MIDPOINTS).tolist() == [0, 0, 1, 0]
    assert M.brute_values(seg, [(100, +1)], 10, 2) == [5, 10, 10, 2] and M.brute_values(seg, [(100, -1)], 10, 2) == [1, 10, 10, 6]
    # both at one position, and a second anchor whose window overlaps the first's: multiplicity
    assert M.values(seg, [(100, +1), (100, -1)], 10, 2).tolist() == [6, 20, 20, 8]
    assert M.values(seg, [(100, +1), (105, +1)], 10, 2).tolist() == [15, 20, 17, 2]


def test_window_is_asymmetric_by_strand():
    """a plus anchor's window is [a - R, a + R), a minus anchor's (a - R, a + R]"""
    assert M.bin_of(80, 100, +1, 10, 2) == 0 and M.bin_of(79, 100, +1, 10, 2) is None and M.bin_of(120, 100, +1, 10, 2) is None
    assert M.bin_of(119, 100, +1, 10, 2) == 3 and M.bin_of(100, 100, +1, 10, 2) == 2 and M.bin_of(99, 100, +1, 10, 2) == 1
    assert M.bin_of(120, 100, -1, 10, 2) == 0 and M.bin_of(121, 100, -1, 10, 2) is None and M.bin_of(80, 100, -1, 10, 2) is None
    assert M.bin_of(81, 100, -1, 10, 2) == 3 and M.bin_of(100, 100, -1, 10, 2) == 2 and M.bin_of(101, 100, -1, 10, 2) == 1


def test_values_are_the_definition():
    r = random.Random(3)
    for _ in range(300):
        w, H = r.choice([1, 2, 3, 7, 10]), r.choice([1, 2, 5, 8])
        L = M.random_normalized(r, r.randint(0, 12), 400, 25)
        anchors = sorted(set((r.randrange(0, 400), r.choice([+1, -1])) for _ in range(r.randint(0, 6))))
        for mode in (M.BASES, M.MIDPOINTS):
            assert M.values(L, anchors, w, H, mode).tolist() == M.brute_values(L, anchors, w, H, mode), (L, anchors, w, H, mode)


def test_far_coordinates():
    """a at 0 and at 2^32 - 1 with R = 2^31: a - R is negative and a + R passes 2^32"""
    top, R = 2 ** 32 - 1, 2 ** 31
    whole = [(0, top)]
    assert M.values(whole, [(0, +1)], R, 1).tolist() == [0, R]
    assert M.values(whole, [(0, -1)], R, 1).tolist() == [R, 1]
    assert M.values(whole, [(top, +1)], R, 1).tolist() == [R, 0]
    assert M.values(whole, [(top, -1)], R, 1).tolist() == [0, R - 1]
    assert M.values([(top - 1, top)], [(top, -1)], 2 ** 30, 2).tolist() == [0, 0, 1, 0]


def test_bounds():
    """0 <= v <= K_t * w in both modes: the list is disjoint, so one anchor sends at most w bases into a bin"""
    r = random.Random(5)
    for _ in range(100):
        w, H = r.choice([1, 3, 10]), r.choice([1, 4])
        lists = [[M.random_normalized(r, 30, 300, 40) for _ in range(2)] for _ in range(3)]
        anchors = [[sorted(set((r.randrange(0, 300), r.choice([+1, -1])) for _ in range(r.randint(0, 5)))) for _ in range(2)] for _ in range(2)]
        for mode in (M.BASES, M.MIDPOINTS):
            v = M.all_values(lists, anchors, w, H, mode)
            assert v.shape == (3, 2, 2 * H) and v.min() >= 0
            for t in range(2):
                assert v[:, t].max() <= sum(len(a) for a in anchors[t]) * w
    # a list that covers every window whole reaches the bound in every bin
    assert M.all_values([[[(0, 1000)]]], [[[(100, +1), (500, -1), (500, +1)]]], 10, 3)[0, 0].tolist() == [30] * 6


def test_words_add_up_over_a_split_and_finish():
    r = np.random.RandomState(7)
    v = r.randint(0, 4, size=(11, 3, 8)).astype(np.int64) * r.randint(0, 2, size=(11, 3, 8))
    obs = r.randint(0, 4, size=(3, 8)).astype(np.int64)
    whole = M.words(v, obs)
    assert np.array_equal(M.words(v[:4], obs) + M.words(v[4:], obs), whole)
    assert whole[..., 0].max() <= 11 and (whole[..., 3] + whole[..., 4] <= 11).all()
    # what a kernel counts -- the samples with v > 0 only -- completed by k_null_finish
    partial = whole.copy()
    partial[..., 3] = ((v < obs[None]) & (v > 0)).sum(axis=0)
    partial[..., 4] = ((v == obs[None]) & (v > 0)).sum(axis=0)
    assert np.array_equal(M.finish(partial, obs, 11), whole)
    assert M.finish(np.zeros((1, 5), dtype=np.int64), [0], 9).tolist() == [[0, 0, 0, 0, 9]]
    assert M.finish(np.zeros((1, 5), dtype=np.int64), [2], 9).tolist() == [[0, 0, 0, 9, 0]]
    # sumsq passes 2^63 and comes back modulo 2^64
    big = np.full((3, 1, 1), 2 ** 31 + 5, dtype=np.int64)
    assert int(M.words(big, np.zeros((1, 1), dtype=np.int64))[0, 0, 2]) % 2 ** 64 == 3 * (2 ** 31 + 5) ** 2
