"""CPU: the model of the relative distance values (tests/reldist_model.py) against the definition by a scan in Python integers,
the hand cases of tests/reldist_cases.py being what they claim to be, the words' additivity over the samples, the bounds the
header states for the area's 64-bit route, and the three point choices of gat-reldist ascending strictly."""
import random

import numpy as np

import reldist_cases as RC
import reldist_model as M
from local_model import random_normalized

TOP = RC.TOP


def scan_values(per_list, per_track, B):
    """the W values of one (list, track) from one_segment alone"""
    hist, outside = [0] * B, 0
    for g in range(len(per_track)):
        for s, e in M.pairs(per_list[g]).tolist():
            k = M.one_segment(s, e, per_track[g], B)
            if k == "outside":
                outside += 1
            elif k is not None:
                hist[k] += 1
    return hist + [M.area_of(hist), sum(hist), outside]


def test_values_follow_the_definition():
    for name, lists, points, bins in RC.hand_geometry():
        assert len(lists) <= 6 and len(points) <= 3 and all(len(l) <= 3 for l in lists), name
        assert all(all(x < y for x, y in zip(g, g[1:])) and all(0 <= x <= TOP for x in g) for t in points for g in t), name
        for B in bins:
            got = M.values(lists, points, B)
            assert got.shape == (len(lists), len(points), B + 3)
            for l in range(len(lists)):
                for t in range(len(points)):
                    assert got[l, t].tolist() == scan_values(lists[l], points[t], B), (name, B, l, t)


def test_hand_cases_are_what_they_say():
    by_name = {c[0]: c for c in RC.hand_geometry()}
    _, lists, points, _ = by_name["example"]
    v = M.values(lists, points, 10)[:, 0]
    # m = 140: d = 40 of 100, bin 8; m = 150: 0.5 itself, the last bin; m = 100: d = 0; m = 200 = p_{K-1}: outside
    assert [int(np.argmax(v[l, :10])) for l in range(3)] == [8, 9, 0] and v[:, 11].tolist() == [1, 1, 1, 0] and v[:, 12].tolist() == [0, 0, 0, 1]
    # one segment, n = 1: all the mass in bin 8.  D = sum_b |10 [b >= 8] - (b + 1)| of n B B = 100
    assert v[0, 10] == sum(abs(10 * (b >= 8) - (b + 1)) for b in range(10)) * 10 ** 6 // 100 and v[3, 10] == 0

    _, lists, points, bins = by_name["lengths"]
    assert [len(l[0]) for l in lists] == list(RC.LENGTHS) and [[len(g) for g in t] for t in points] == [[17, 1, 0], [4, 5, 2], [0, 0, 0]]
    assert [len(l[1]) > 0 for l in lists] == [False, True] * 3 and all(len(l[2]) == 20 for l in lists)
    assert tuple(bins) == (1, 2, 64, 66, 1024)
    v = M.values(lists, points, 64)
    assert (v[:, 2, :66] == 0).all() and v[:, 2, 66].tolist() == [20, 30, 83, 93, 85, 159]      # the empty track: everything outside
    assert v[0, 0, 66] == 20 and v[0, 0, 65] == 0                 # list 0: only group 2 holds segments, where track 0 has no point
    assert (v[1:, 0, 65] > 0).all() and (v[:, 1, 65] > 0).all()   # inside somewhere
    # track 1, group 1: the points lie beyond every segment
    assert all(M.one_segment(s, e, points[1][1], 64) == "outside" for l in lists for s, e in l[1])
    assert any(any(a < s for a in starts[:k]) for l in lists for starts in ([s for s, _ in l[0]],) for k, s in enumerate(starts))   # unsorted

    _, lists, points, _ = by_name["edges"]
    P = points[0][0]
    assert len(lists) == 5 and P[1] - P[0] == 1 and (P[3] - P[2]) % 2 == 0
    for B in (1, 2, 3, 50, 64, 1024):
        f = lambda s, e, t=0: M.one_segment(s, e, points[t][0], B)      # noqa: E731
        assert f(100, 101) == 0 and f(200, 201) == "outside" and f(110, 111) == 0         # gap == 1 / m == p_{K-1} / d == 0
        assert f(115, 116) == f(114, 117) == B - 1 and 2 * 5 * B // 10 == B               # the centre: the clamp to B - 1
        assert f(105, 107) == min(B - 1, 2 * 4 * B // 9) and f(119, 120) == 2 * 1 * B // 10
        assert f(50, 50) is None and f(60, 40) is None and f(10, 20) == f(300, 400) == "outside"
        assert f(110, 111, 1) == f(100, 130, 1) == "outside"                              # K < 2
        assert f(115, 116, 2) == 0 and f(116, 117, 2) == "outside"
        v = M.values(lists, points, B)
        assert v[:, 0, B + 1].tolist() == [2, 4, 0, 5, 0] and v[:, 0, B + 2].tolist() == [1, 0, 2, 0, 0] and v[4].sum() == 0
        assert v[:, 1, B + 1].sum() == 0 and v[:, 1, B + 2].tolist() == [3, 4, 2, 5, 0]
    assert not all(a <= b for a, b in zip(lists[3][0], lists[3][0][1:])) and lists[3][0][0] == lists[3][0][3]

    _, lists, points, _ = by_name["far"]
    assert points[0][0] == [0, TOP]
    for B in (1, 2, 64, 66, 1024):
        f = lambda s, e: M.one_segment(s, e, [0, TOP], B)      # noqa: E731
        assert f(0, 1) == 0 and f(TOP - 1, TOP) == 0 and f(2 ** 31 - 1, 2 ** 31 + 1) == B - 1 and f(0, TOP) == B - 1
        assert f(2 ** 30, 2 ** 30 + 1) == (2 ** 31 * B) // TOP
    assert 2 * 2 ** 30 * 1024 >= 2 ** 32 and M.one_segment(2 ** 30, 2 ** 30 + 1, [0, TOP], 1024) == 512       # (32 bits would give 0)
    v = M.values(lists, points, 2)
    # bins 0, 0, 1, 1 (2^32 // (2^32 - 1)), 1: C = 2, 5 and D = |2 * 2 - 5| + |2 * 5 - 10| = 1 of n B B = 20; group 1 has one point
    assert v[0, 0].tolist() == [2, 3, 50000, 5, 1] and v[:, 2, 2 + 2].tolist() == [6, 4]


def test_area():
    r = random.Random(9)
    for B in (1, 2, 3, 50, 1024):
        for _ in range(20):
            hist = [r.choice([0, 0, 1, 5, r.randrange(0, 10 ** 6)]) for _ in range(B)]
            assert 0 <= M.area_of(hist) <= M.AREA_SCALE            # (area_of forms it both ways and compares)
        assert M.area_of([0] * B) == 0
        uniform = M.area_of([7] * B)
        assert uniform == 0                                        # the uniform histogram: C_b = (b + 1) n / B
        first, last = M.area_of([9] + [0] * (B - 1)), M.area_of([0] * (B - 1) + [9])
        # all the mass in bin 0: D = n sum_b (B - b - 1) = n B (B - 1) / 2; in the last bin: D = n sum_{b < B - 1} (b + 1), the same
        assert first == last == (B - 1) * 10 ** 6 // (2 * B)
    # the stated bounds at n = 2^31 - 1, B = 1024: M < 2^51, D <= M, no intermediate reaches 2^61
    n, B = 2 ** 31 - 1, 1024
    for hist in ([n] + [0] * (B - 1), [0] * (B - 1) + [n], [n // B] * (B - 1) + [n - (B - 1) * (n // B)], [0] * 511 + [n - 5, 5] + [0] * 511):
        C = D = 0
        for b in range(B):
            C += hist[b]
            D += abs(B * C - (b + 1) * n)
        seen = []
        got = M.area_route(D, n, B, seen)
        assert n * B * B < 2 ** 51 and D <= n * B * B and max(seen) < M.LIMIT and got == D * 10 ** 6 // (n * B * B) <= 10 ** 6
    # ... and at the largest D there is: D == M would be r = 1000 M
    seen = []
    assert M.area_route(n * B * B, n, B, seen) == 10 ** 6 and max(seen) < M.LIMIT


def test_words_are_additive():
    r = random.Random(4)
    points = [[RC.spread_points(r, 9, 500)], [[100, 400]]]
    lists = [[RC.any_segments(r, r.randrange(0, 30), 500, 20)] for _ in range(12)]
    v = M.values(lists, points, 7)
    assert v.shape == (12, 2, 10) and (v[..., 8] > 0).any() and (v[..., 9] > 0).any()
    obs = v[3].copy()
    obs[:, ::3] += 1
    whole = M.words(v, obs)
    for k in (0, 1, 5, 12):
        assert np.array_equal(M.words(v[:k], obs) + M.words(v[k:], obs), whole)
    assert whole[..., 0].max() <= 12 and (whole[..., 3] + whole[..., 4] <= 12).all()


def test_point_choices_ascend():
    """disjoint non-empty intervals give strictly ascending midpoints, starts and last bases"""
    from gat_amd import reldist
    r = random.Random(12)
    for _ in range(50):
        span = r.choice([40, 1000, 10 ** 6])
        iv = random_normalized(r, r.randrange(0, 40), span, r.choice([1, 2, 30]))
        a = np.zeros(len(iv), dtype=[("start", "<u4"), ("end", "<u4")])
        if iv:
            a["start"], a["end"] = np.array(iv, dtype=np.int64).T
        for point, f in (("midpoint", lambda s, e: s + (e - s) // 2), ("start", lambda s, e: s), ("end", lambda s, e: e - 1)):
            got = reldist.points_of(a, point)
            assert got.dtype == np.uint32 and got.tolist() == [f(s, e) for s, e in iv]
            assert all(x < y for x, y in zip(got.tolist(), got.tolist()[1:]))
    top = np.array([(TOP - 1, TOP)], dtype=[("start", "<u4"), ("end", "<u4")])
    assert [int(reldist.points_of(top, p)[0]) for p in reldist.ANNOTATION_POINTS] == [TOP - 1, TOP - 1, TOP - 1]
