"""CPU: the numpy model of the pair hits (tests/pairs_model.py) against the definition -- every segment against every interval
-- on random normalized and unnormalized lists, its diagonal against the oracle's intersectionWithSegments on normalized lists,
and its five words against plain Python on the rows of sample values."""
import random

import numpy as np

from oracle import oracle as O

import pairs_model as M


def _random_list(r, normalized, span=300):
    if normalized:
        return M.random_normalized(r, r.choice([0, 1, 3, 12]), span, max_len=r.choice([1, 5, 60]))
    out = [(s, s + r.choice([-2, 0, 1, 1, 5, 40, 120])) for s in (r.randrange(2, span) for _ in range(r.choice([0, 1, 4, 15])))]
    return out                                   # unsorted, overlapping, and some with e <= s


def test_counts_equal_the_definition():
    r = random.Random(19)
    seen_partial = seen_skipped = False
    for case in range(120):
        T, G = r.choice([1, 2, 3, 5]), r.choice([1, 2, 3])
        tracks = [[M.random_normalized(r, r.choice([0, 1, 4, 15]), 300, max_len=r.choice([1, 5, 60])) for _ in range(G)] for _ in range(T)]
        assert all(M.is_normalized(a) for t in tracks for a in t)
        per_list = [_random_list(r, case % 2 == 0) for _ in range(G)]
        got = M.counts(per_list, tracks)
        want = M.brute_counts(per_list, tracks)
        assert got.dtype == np.int64 and got.tolist() == want, (per_list, tracks)
        c = dict(zip(M.pair_list(T), want))
        seen_partial |= any(0 < c[i, j] < min(c[i, i], c[j, j]) for i, j in c if i < j)
        seen_skipped |= any(e <= s for seg in per_list for s, e in seg)
    assert seen_partial and seen_skipped


def test_hand_hits():
    A = [(10, 20), (20, 30), (50, 60)]
    # bookended on either side: no hit; one shared base: a hit; over several intervals: one hit; empty and reversed: skipped
    L = [(0, 10), (0, 11), (30, 50), (29, 30), (60, 70), (59, 60), (5, 100), (15, 15), (18, 12)]
    assert M.hits(L, A).tolist() == [False, True, False, True, False, True, True, False, False]
    assert M.hits(L, []).tolist() == [False] * len(L) and M.hits([], A).tolist() == []
    top = 2 ** 32 - 1
    assert M.hits([(top - 1, top), (0, top), (top - 2, top - 1)], [(top - 1, top)]).tolist() == [True, True, False]
    # two tracks, two groups: the pairs in their order, the counts summed over the groups
    tracks = [[[(0, 10)], [(0, 10)]], [[(5, 15)], []]]
    assert M.pair_list(2) == [(0, 0), (0, 1), (1, 1)]
    assert M.counts([[(0, 5), (6, 7), (12, 13)], [(1, 2)]], tracks).tolist() == [3, 1, 2]


def test_diagonal_is_the_reference_segment_overlap():
    r = random.Random(23)
    nonzero = 0
    for _ in range(200):
        L = M.random_normalized(r, r.choice([0, 1, 3, 12]), 300, max_len=r.choice([1, 5, 60]))
        tracks = [[M.random_normalized(r, r.choice([0, 1, 4, 15]), 300, max_len=r.choice([1, 5, 60]))] for _ in range(3)]
        c = dict(zip(M.pair_list(3), M.counts([L], tracks).tolist()))
        for t in range(3):
            want = O.intersection_with_segments(L, tracks[t][0], "base")
            assert c[t, t] == want, (L, tracks[t][0])
            nonzero += want > 0
    assert nonzero > 100


def test_words_of_pair_counts():
    r = random.Random(5)
    v = np.array([[r.choice([0, 0, 0, 1, 5, 9]) for _ in range(6)] for _ in range(13)], dtype=np.int64)
    obs = np.array([0, 1, 5, 9, 3, 100], dtype=np.int64)
    w = M.words(v, obs)
    assert w.shape == (6, 5)
    for k in range(6):
        row, o = v[:, k].tolist(), int(obs[k])
        assert w[k].tolist() == [sum(1 for x in row if x > 0), sum(row), sum(x * x for x in row), sum(1 for x in row if x < o),
                                 sum(1 for x in row if x == o)]
    assert np.array_equal(M.words(v[:4], obs) + M.words(v[4:], obs), w)


def test_from_sample_and_csr_layout():
    seg, off = M.csr([[[(0, 4), (5, 9)], []], [[], [(2, 3)]]])
    assert off.tolist() == [0, 2, 2, 2, 3] and seg["start"].tolist() == [0, 5, 2] and seg["end"].tolist() == [4, 9, 3]
    tracks = [[[(0, 5)], [(0, 100)]], [[(3, 6)], []]]
    assert M.from_sample(seg, off, 2, tracks).tolist() == [[1, 1, 2], [1, 0, 0]]
