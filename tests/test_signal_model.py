"""CPU: the model of k_signal (tests/signal_model.py) on its hand cases, against a count base by base, and the two ways the
four words add up: over a split of the segment list and over the groups."""
import random

import numpy as np

import signal_model as M


def test_hand_cases():
    for name, segs, pieces, values, want in M.HAND:
        assert M.is_normalized(pieces), name
        assert M.words(segs, pieces, values) == want, name
    names = [h[0] for h in M.HAND]
    assert len(set(names)) == len(names) >= 18


def test_what_the_hand_cases_cover():
    by = {h[0]: h[4] for h in M.HAND}
    n, covered, hit, total = by["adjacent pieces of opposite sign that cancel"]
    assert total == 0 and covered > 0 and hit == 1
    assert by["bookended on the left of a piece: no hit"][1:] == by["bookended on the right of a piece: no hit"][1:] == [0, 0, 0]
    assert by["a one-base overlap at the start"][1] == by["a one-base overlap at the end"][1] == 1
    assert by["segments of no length are skipped"][0] == 1 and by["no pieces"] == [2, 0, 0, 0]
    assert by["pieces of value 0 are covered and hit"] == [1, 20, 1, 0]
    assert by["the largest value over a long piece"][3] > 2 ** 62 and by["the most negative value over a long piece"][3] < -2 ** 61


def test_against_a_count_base_by_base():
    r = random.Random(11)
    for _ in range(300):
        pieces, values = M.random_pieces(r, r.choice([0, 1, 2, 5, 9]), 120, max_len=8)
        top = (pieces[-1][1] if pieces else 30) + 10
        per_base = np.zeros(top + 80, dtype=np.int64)
        has = np.zeros(top + 80, dtype=bool)
        for (a, b), q in zip(pieces, values):
            per_base[a:b] = q
            has[a:b] = True
        segs = M.random_segments(r, 6, top, max_len=40)
        n = covered = hit = total = 0
        for s, e in segs:
            if e > s:
                n += 1
                covered += int(has[s:e].sum())
                hit += int(has[s:e].any())
                total += int(per_base[s:e].sum())
        assert M.words(segs, pieces, values) == [n, covered, hit, total]


def test_words_add_over_a_split_of_the_list_and_over_groups():
    r = random.Random(5)
    groups = []
    for g in range(3):
        pieces, values = M.random_pieces(r, 12, 400)
        groups.append((M.random_segments(r, 30, 450), pieces, values))
    whole = [0, 0, 0, 0]
    for segs, pieces, values in groups:
        w = M.words(segs, pieces, values)
        for cut in (0, 1, 13, 30):
            a, b = M.words(segs[:cut], pieces, values), M.words(segs[cut:], pieces, values)
            assert [x + y for x, y in zip(a, b)] == w, cut
        whole = [x + y for x, y in zip(whole, w)]
    assert M.pair_words([g[0] for g in groups], [(g[1], g[2]) for g in groups]) == whole
    got = M.all_words([[g[0] for g in groups], [[], [], []]], [[(g[1], g[2]) for g in groups]])
    assert got.shape == (2, 1, 4) and got[0, 0].tolist() == whole and got[1, 0].tolist() == [0, 0, 0, 0]


def test_from_sample_cuts_the_lists_by_contig():
    seg = np.zeros(5, dtype=[("start", "<u4"), ("end", "<u4")])
    seg["start"], seg["end"] = [0, 10, 5, 7, 0], [4, 20, 6, 9, 100]
    off = np.array([0, 2, 3, 4, 5], dtype=np.int64)               # two samples, two contigs
    tracks = [[([(0, 50)], [2]), ([(0, 6)], [-1])]]
    got = M.from_sample(seg, off, 2, tracks)
    assert got.tolist() == [[[3, 15, 3, 27]], [[2, 8, 2, -2]]]
