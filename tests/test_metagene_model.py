"""The model of the metagene along scaled features (tests/metagene_model.py) against the definition base by base, the worked
example of include/gat_mi355.h, the mirror property of a minus feature, the stated bounds, the hand-made cases of
tests/metagene_cases.py being what their names say, and the arithmetic of the five words: additive over a split of the
samples.  No GPU."""
import random

import numpy as np

import metagene_cases as MC
import metagene_model as M


def test_worked_example():
    seg = [(95, 112)]
    assert M.values(seg, [(100, 110, +1)], 4, 1, 10).tolist() == [5, 3, 2, 3, 2, 2]
    assert M.values(seg, [(100, 110, -1)], 4, 1, 10).tolist() == [2, 3, 2, 3, 2, 5]
    assert M.values(seg, [(100, 110, +1)], 4, 1, 10, M.MIDPOINTS).tolist() == [0, 0, 1, 0, 0, 0]
    assert M.values(seg, [(100, 110, -1)], 4, 1, 10, M.MIDPOINTS).tolist() == [0, 0, 0, 1, 0, 0]
    assert M.brute_values(seg, [(100, 110, +1)], 4, 1, 10) == [5, 3, 2, 3, 2, 2] and M.brute_values(seg, [(100, 110, -1)], 4, 1, 10) == [2, 3, 2, 3, 2, 5]
    # body bins of unequal width: 10 bases over 4 bins are 3, 2, 3, 2 -- bin k holds [ceil(10 k / 4), ceil(10 (k + 1) / 4))
    lo, hi = M.bin_bases(100, 110, +1, 4, 0, 1)
    assert lo.tolist() == [100, 103, 105, 108] and hi.tolist() == [103, 105, 108, 110]
    lo, hi = M.bin_bases(100, 110, -1, 4, 0, 1)
    assert lo.tolist() == [107, 105, 102, 100] and hi.tolist() == [110, 107, 105, 102]
    # a nested feature and one span on both strands: multiplicity
    assert M.values(seg, [(100, 110, +1), (100, 110, -1)], 4, 1, 10).tolist() == [7, 6, 4, 6, 4, 7]
    assert M.values([(0, 200)], [(100, 110, +1), (104, 106, -1)], 2, 1, 3).tolist() == [6, 6, 6, 6]
    # a feature shorter than its body bins: 3 bases over 5 bins fill the bins floor(5 o / 3) = 0, 1, 3 and leave 2 and 4 empty
    assert M.values([(0, 50)], [(10, 13, +1)], 5, 0, 1).tolist() == [1, 1, 0, 1, 0]
    assert [M.bin_of(x, 10, 13, +1, 5, 0, 1) for x in (10, 11, 12)] == [0, 1, 3]


def test_the_window_is_one_on_both_strands():
    """the mirror maps the window onto itself: [fs - F, fe + F) on either strand, without a shift by a base"""
    for sigma in (+1, -1):
        assert M.bin_of(79, 100, 110, sigma, 4, 2, 10) is None and M.bin_of(130, 100, 110, sigma, 4, 2, 10) is None
        assert M.bin_of(80, 100, 110, sigma, 4, 2, 10) == (0 if sigma > 0 else 7) and M.bin_of(129, 100, 110, sigma, 4, 2, 10) == (7 if sigma > 0 else 0)
    assert [M.bin_of(x, 100, 110, +1, 4, 2, 10) for x in (99, 100, 109, 110)] == [1, 2, 5, 6]
    assert [M.bin_of(x, 100, 110, -1, 4, 2, 10) for x in (99, 100, 109, 110)] == [6, 5, 2, 1]


def random_features(r, n, span, max_len):
    return sorted(set((s, s + r.randint(1, max_len), r.choice([+1, -1])) for s in (r.randrange(0, span) for _ in range(n))), key=M.feature_key)


def test_values_are_the_definition():
    r = random.Random(3)
    for _ in range(300):
        Bb, Bf, w = r.choice([1, 2, 3, 7, 10, 40]), r.choice([0, 1, 2, 5]), r.choice([1, 2, 3, 7])
        L = M.random_normalized(r, r.randint(0, 12), 400, 25)
        features = random_features(r, r.randint(0, 6), 400, r.choice([1, 5, 30, 200]))
        for mode in (M.BASES, M.MIDPOINTS):
            assert M.values(L, features, Bb, Bf, w, mode).tolist() == M.brute_values(L, features, Bb, Bf, w, mode), (L, features, Bb, Bf, w, mode)


def test_a_minus_feature_is_the_mirror():
    """bin(x; -) = bin(fs + fe - 1 - x; +): the row of a minus feature is the row of the plus feature against the segments mirrored
    through fs + fe - 1, and -- where the body bins are equally wide, so that the bins are symmetric -- the reversed row of the
    plus feature against the same segments"""
    r = random.Random(11)
    for _ in range(200):
        Bb, Bf, w = r.choice([1, 3, 8, 33]), r.choice([0, 1, 4]), r.choice([1, 3, 10])
        fs = r.randrange(400, 500)
        fe = fs + r.randint(1, 120)
        L = M.random_normalized(r, r.randint(1, 15), 700, 30)
        mirrored = sorted((fs + fe - e, fs + fe - s) for s, e in M.pairs(L).tolist())       # x -> fs + fe - 1 - x on [s, e)
        assert all(s >= 0 for s, _ in mirrored) and M.is_normalized(mirrored)
        for mode in (M.BASES,) + ((M.MIDPOINTS,) if all((e - s) % 2 for s, e in mirrored) else ()):     # (an odd length keeps its midpoint)
            minus = M.values(L, [(fs, fe, -1)], Bb, Bf, w, mode)
            assert minus.tolist() == M.values(mirrored, [(fs, fe, +1)], Bb, Bf, w, mode).tolist()
            # where the body bins are equally wide the bins themselves are symmetric: the same segments give the reversed row
            if (fe - fs) % Bb == 0:
                assert minus.tolist() == M.values(L, [(fs, fe, +1)], Bb, Bf, w, mode).tolist()[::-1]
        assert minus.sum() > 0 or not any(e > fs - Bf * w and s < fe + Bf * w for s, e in M.pairs(L).tolist())


def test_far_coordinates():
    """fs = 0 and fe = 2^32 - 1 with F = 2^31: fs - F is negative and fe + F passes 2^32"""
    top, F = MC.TOP, 2 ** 31
    whole = [(0, top)]
    assert M.values(whole, [(0, top, +1)], 1, 1, F).tolist() == [0, top, 0]
    assert M.values(whole, [(0, 7, +1)], 1, 1, F).tolist() == [0, 7, F]
    assert M.values(whole, [(0, 7, -1)], 1, 1, F).tolist() == [F, 7, 0]
    assert M.values(whole, [(top - 4, top, +1)], 2, 1, F).tolist() == [F, 2, 2, 0]
    assert M.values([(top - 1, top)], [(0, top, -1)], 4, 1, F).tolist() == [0, 1, 0, 0, 0, 0]
    assert M.values([(2 ** 31, 2 ** 31 + 1)], [(0, top, +1)], 1000, 0, 1).tolist() == [0] * 500 + [1] + [0] * 499


def test_bounds():
    """0 <= v; a flank cell is at most K_t * w and a body cell at most sum_f ceil(len_f / Bb) in both modes: the list is
    disjoint, so one feature sends at most w bases into a flank bin and ceil(len / Bb) into a body bin"""
    r = random.Random(5)
    for _ in range(100):
        Bb, Bf, w = r.choice([1, 3, 10]), r.choice([0, 1, 4]), r.choice([1, 3, 10])
        lists = [[M.random_normalized(r, 30, 300, 40) for _ in range(2)] for _ in range(3)]
        features = [[random_features(r, r.randint(0, 5), 300, 60) for _ in range(2)] for _ in range(2)]
        most = M.bounds(features, Bb, Bf, w)
        for mode in (M.BASES, M.MIDPOINTS):
            v = M.all_values(lists, features, Bb, Bf, w, mode)
            assert v.shape == (3, 2, 2 * Bf + Bb) and v.min() >= 0
            for t in range(2):
                flat = [f for g in features[t] for f in g]
                flank = np.concatenate([v[:, t, :Bf], v[:, t, Bf + Bb:]], axis=1)
                assert flank.size == 0 or flank.max() <= len(flat) * w
                assert v[:, t, Bf:Bf + Bb].max() <= sum(-(-(fe - fs) // Bb) for fs, fe, _ in flat)
                assert v[:, t].max() <= most[t]
    # a list that covers every window whole reaches both bounds
    got = M.all_values([[[(0, 1000)]]], [[[(100, 110, +1), (500, 507, -1), (500, 507, +1)]]], 3, 2, 10)[0, 0]
    assert got.tolist() == [30, 30, 4 + 3 + 3, 3 + 2 + 2, 3 + 2 + 2, 30, 30] and M.bounds([[[(100, 110, +1), (500, 507, -1), (500, 507, +1)]]], 3, 2, 10) == [30]
    assert M.bounds([[[(0, 100, +1)], [(5, 6, -1)]]], 7, 0, 2 ** 31) == [15 + 1]         # (without flanks w does not count)


def test_hand_geometry_is_what_it_says():
    by_name = {c[0]: c for c in MC.hand_geometry()}
    for name, lists, features, geometries in by_name.values():
        assert len(lists) <= 6 and len(features) <= 3 and all(len(l) <= 3 and all(M.is_normalized(x) for x in l) for l in lists), name
        for keys in ([M.feature_key(f) for f in g] for t in features for g in t):          # ascending by (start, end, minus), none twice
            assert all(x < y for x, y in zip(keys, keys[1:])), name
        for Bb, Bf, w in geometries:
            assert 2 * Bf + Bb <= 1024 and Bf * w <= 2 ** 31 and max(M.bounds(features, Bb, Bf, w)) < 2 ** 32, name
    _, lists, features, ((Bb, Bf, w),) = by_name["example"]
    assert M.all_values(lists, features, Bb, Bf, w)[0].tolist() == [[5, 3, 2, 3, 2, 2], [2, 3, 2, 3, 2, 5], [7, 6, 4, 6, 4, 7]]
    assert M.all_values(lists, features, Bb, Bf, w, M.MIDPOINTS)[0].tolist() == [[0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 0, 0], [0, 0, 1, 1, 0, 0]]
    _, lists, features, geometries = by_name["lengths"]
    assert [len(l[0]) for l in lists] == list(MC.LENGTHS) and [[len(g) for g in t] for t in features] == [[17, 1, 0], [4, 5, 4], [0, 0, 0]]
    assert [bool(l[1]) for l in lists] == [False, True] * 3 and all(l[2] for l in lists)
    assert geometries == ((1, 0, 1), (64, 0, 1), (2, 32, 3), (66, 0, 1), (10, 507, 1))
    f17 = features[0][0]
    assert any(a[0] == b[0] and a[1] < b[1] for a, b in zip(f17, f17[1:]))                  # equal starts with different ends
    assert any(a[:2] == b[:2] for a, b in zip(f17, f17[1:]))                               # one span on both strands
    assert any(b[1] < a[1] for a, b in zip(f17, f17[1:]))                                  # the ends do not ascend
    _, lists, features, geometries = by_name["short-features"]
    assert geometries[0] == (1024, 0, 1) and sorted(set(fe - fs for fs, fe, _ in features[0][0])) == [1, 3]
    want = M.all_values(lists, features, 1024, 0, 1)
    # the base 10: the one base of (10, 11, +), and the last of (10, 13, -) in the direction of its strand, floor(2 * 1024 / 3)
    assert np.flatnonzero(want[2, 0]).tolist() == [0, 682] and want[2, 0, 0] == 1 and want[2, 0, 682] == 1
    assert want[1, 1].tolist() == [1] + [0] * 1023
    _, lists, features, _ = by_name["nested"]
    (both,), (short,) = features
    assert len(both) == 17 and len(short) == 16 and both[0] == (200, 3000, +1) and all(both[0][0] < fs and fe < both[0][1] for fs, fe, _ in short)
    lo, hi = min(fs for fs, _, _ in short), max(fe for _, fe, _ in short)
    assert [("left" if e <= lo else "right" if s >= hi else "inside") for s, e in lists[0][0]] == ["left", "left", "inside"]
    assert all(s < hi and e > lo for s, e in lists[1][0]) and lists[2][0][0][0] >= hi
    want = M.all_values(lists, features, 8, 0, 1)
    assert want[2, 1].sum() == 0 and want[2, 0].sum() == 10 + 10 and want[0, 1].sum() == 1 and want[0, 0].sum() == 0 + 20 + 11 + 1
    _, lists, features, _ = by_name["overlapping-windows"]
    assert M.all_values(lists, features, 3, 0, 1)[0, 0].tolist() == [7 + 20 + 20 + 5 + 24, 7 + 20 + 20 + 5 + 23, 6 + 20 + 20 + 5 + 23]
    assert M.all_values(lists, features, 7, 5, 10)[0, 0, :5].tolist() == [50] * 5           # every flank bin whole, once per feature
    _, lists, features, _ = by_name["bookended"]
    want = M.all_values(lists, features, 4, 2, 10)
    assert want[0].sum() == 0
    assert want[1, 0].tolist() == [5, 0, 0, 0, 0, 0, 0, 5] == want[1, 1].tolist()
    assert want[2, 0].tolist() == [0, 5, 0, 0, 0, 0, 5, 0] == want[2, 1].tolist()
    assert want[3, 0].tolist() == [0, 0, 3, 0, 0, 3, 0, 0] == want[3, 1].tolist()
    assert want[4, 0].tolist() == [0, 10, 10, 0, 0, 10, 10, 0]
    _, lists, features, _ = by_name["far-plus"]
    assert M.all_values(lists, features, 1, 1, 2 ** 31)[0].tolist() == [[0, MC.TOP, 0], [0, 7, 2 ** 31], [0, 0, 0]]
    _, lists, features, _ = by_name["far-minus"]
    assert M.all_values(lists, features, 1, 1, 2 ** 31)[0].tolist() == [[0, MC.TOP, 0], [2 ** 31, 7, 0], [0, 0, 0]]


def test_words_add_up_over_a_split():
    r = np.random.RandomState(7)
    v = r.randint(0, 4, size=(11, 3, 8)).astype(np.int64) * r.randint(0, 2, size=(11, 3, 8))
    obs = r.randint(0, 4, size=(3, 8)).astype(np.int64)
    whole = M.words(v, obs)
    assert np.array_equal(M.words(v[:4], obs) + M.words(v[4:], obs), whole)
    assert whole[..., 0].max() <= 11 and (whole[..., 3] + whole[..., 4] <= 11).all()
    partial = whole.copy()
    partial[..., 3] = ((v < obs[None]) & (v > 0)).sum(axis=0)
    partial[..., 4] = ((v == obs[None]) & (v > 0)).sum(axis=0)
    assert np.array_equal(M.finish(partial, obs, 11), whole)
