"""CPU: the model of k_distance (tests/distance_model.py) against the definition taken literally -- the smallest gap over all
pairs, O(n m) -- on hand cases and on random normalized lists with arbitrary queries."""
import random

import numpy as np
import pytest

import distance_model as M


@pytest.mark.parametrize("case", M.HAND, ids=[c[0] for c in M.HAND])
def test_hand_cases(case):
    _, q, t, want = case
    assert M.distances(q, t).tolist() == want
    assert M.brute_force(q, t) == want
    for bound in (0, 1, 40, 2 ** 32):
        assert M.words(q, t, bound) == [len(want), sum(want), sum(1 for d in want if d <= bound), 0]


def test_empty_t_gives_none():
    _, q, t, want = M.EMPTY_T
    assert M.words(q, t, 1000) == want
    assert M.words([], [], 1000) == [0, 0, 0, 0] and M.words([], M.T3, 1000) == [0, 0, 0, 0]


def test_structured_arrays_are_taken_like_pairs():
    from gat_amd import intervals
    q = intervals.make([10, 500, 250], [20, 600, 250])
    t = intervals.make([a for a, _ in M.T3], [b for _, b in M.T3])
    assert M.distances(q, t).tolist() == [81, 51] and M.words(q, t, 60) == [2, 132, 1, 0]


def test_fuzz_against_the_brute_force():
    r = random.Random(15)
    hits = near = far = 0
    for round_ in range(300):
        k = r.choice([1, 2, 3, 10, 40])
        t = M.random_normalized(r, k, r.choice([50, 400, 5000]))
        q = M.random_queries(r, r.choice([0, 1, 5, 30]), t[-1][1] + 100)
        got = M.distances(q, t).tolist()
        assert got == M.brute_force(q, t), (round_, q, t)
        hits += got.count(0)
        near += got.count(1)
        far += sum(1 for d in got if d > 1)
        bound = r.choice([0, 1, 7, 100])
        assert M.words(q, t, bound) == [len(got), sum(got), sum(1 for d in got if d <= bound), 0]
    assert hits > 100 and near > 20 and far > 100


def test_is_normalized():
    assert M.is_normalized([]) and M.is_normalized(M.T3) and M.is_normalized([(0, 1), (1, 2)])
    assert not M.is_normalized([(0, 5), (4, 8)]) and not M.is_normalized([(4, 8), (0, 2)]) and not M.is_normalized([(3, 3)])


def test_pairs_sum_over_the_groups_in_both_directions():
    segs = [[(10, 20), (500, 600)], [(1, 2)], []]
    track = [M.T3, [], [(5, 9)]]
    assert M.pair_words(segs, track, M.SEGMENT_TO_ANNOTATION, 60).tolist() == [2, 132, 1, 1]
    # from the track: its three intervals against the two segments, one interval against nothing, nothing against one segment
    d = M.distances(M.T3, segs[0]).tolist()
    assert d == [81, 101, 51]
    assert M.pair_words(segs, track, M.ANNOTATION_TO_SEGMENT, 60).tolist() == [3, sum(d), 1, 1]
    got = M.all_words([segs, segs], [track], M.SEGMENT_TO_ANNOTATION, 60)
    assert got.shape == (2, 1, 4) and got.dtype == np.int64 and got[0].tolist() == got[1].tolist() == [[2, 132, 1, 1]]
