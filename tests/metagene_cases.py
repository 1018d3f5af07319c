"""Hand-made geometry for the metagene tests (tests/test_metagene_model.py says what each case is, on the CPU;
tests/test_metagene_gpu.py runs them on the device).  TEST INFRASTRUCTURE ONLY.  A case is (name, lists[l][g], features[t][g],
the (body_bins, flank_bins, flank_bin_size) it runs at): at most 3 groups, 3 tracks and 6 lists.  A feature is (start, end,
sigma); within a (track, group) the features ascend by (start, end, minus)."""
import random

from local_model import random_normalized

TOP = 2 ** 32 - 1
LENGTHS = (0, 1, 63, 64, 65, 130)
GEOMETRIES = ((1, 0, 1), (64, 0, 1), (2, 32, 3), (66, 0, 1), (10, 507, 1))


def key(f):
    return (f[0], f[1], 1 if f[2] < 0 else 0)


def spread_features(r, n, span, max_len):
    """n distinct features below span, ascending by (start, end, minus): overlapping ones among them, every fourth pair with
    equal starts and different ends, every fourth other pair one span on both strands"""
    out = set()
    while len(out) < n:
        s = r.randrange(0, span - max_len)
        f = (s, s + r.randint(1, max_len), r.choice([+1, -1]))
        out.add(f)
        if len(out) % 4 == 1 and len(out) < n:
            out.add((f[0], f[1] + r.randint(1, max_len), f[2]))
        elif len(out) % 4 == 3 and len(out) < n:
            out.add((f[0], f[1], -f[2]))
    return sorted(out, key=key)


def hand_geometry():
    cases = []
    # the header's example: body bins of 3, 2, 3 and 2 bases
    cases.append(("example", [[[(95, 112)]]], [[[(100, 110, +1)]], [[(100, 110, -1)]], [[(100, 110, +1), (100, 110, -1)]]], ((4, 1, 10),)))
    # list lengths 0, 1, 63, 64, 65, 130 on group 0 (the lane stride and its tail); features per (track, group) 0, 1, 4, 5, 17 (the
    # staging limit of 4 and the block table); group 1: features, and segments in every other list only; group 2: segments, and
    # track 0 without a feature; track 2 is empty
    r = random.Random(41)
    span = 2000
    lists = []
    for k, n in enumerate(LENGTHS):
        g0 = random_normalized(r, n, span, 12)
        lists.append([g0, random_normalized(r, 9, span, 30) if k % 2 else [], random_normalized(r, 20, span, 5)])
    features = [[spread_features(r, 17, span, 150), [(700, 760, -1)], []],
                [spread_features(r, 4, span, 300), spread_features(r, 5, span, 40), spread_features(r, 4, span, 900)],
                [[], [], []]]
    cases.append(("lengths", lists, features, GEOMETRIES))
    # 1024 body bins over features of 1 and 3 bases: almost every body bin without a base
    tiny = [[[(10, 11, +1), (10, 13, -1), (12, 13, -1), (20, 23, +1)]], [[(11, 12, -1)]]]
    cases.append(("short-features", [[[(9, 12), (12, 14), (21, 22)]], [[(0, 40)]], [[(10, 11)]]], tiny, ((1024, 0, 1), (1018, 3, 2))))
    # nested: one feature over 16 short ones (their ends do not ascend: the prefix maximum of the ends is the long one's from
    # the start), queried left of, inside and right of the short ones -- and a second track with the short ones alone
    short = [(1000 + 20 * k, 1000 + 20 * k + 7 + k % 3, (-1) ** k) for k in range(16)]
    long_one = (200, 3000, +1)
    nested_l = [[[(100, 150), (400, 420), (990, 1001)]], [[(1005, 1012), (1100, 1130), (1306, 1330)]], [[(1400, 1410), (2990, 3005), (3050, 3060)]],
                [[(0, 4000)]]]
    cases.append(("nested", nested_l, [[sorted([long_one] + short, key=key)], [short]], ((8, 0, 1), (5, 3, 4), (3, 30, 2))))
    # equal starts with different ends, one span on both strands, windows of neighbours that overlap, a segment over a whole
    # window and more
    over_l = [[[(0, 1000)]], [[(250, 300), (300, 340), (395, 400)]], [[(349, 350)]]]
    over_f = [[[(300, 320, +1), (300, 360, +1), (300, 360, -1), (330, 345, -1), (350, 420, +1)]], [[(300, 311, -1)]]]
    cases.append(("overlapping-windows", over_l, over_f, ((7, 5, 10), (3, 0, 1), (11, 2, 1))))
    # a segment bookended with each of the four region edges, outside and inside: (1000, 1100) with F = 20 has the window
    # [980, 1120) and the edges 980, 1000, 1100, 1120, on either strand
    book_l = [[[(970, 980), (1120, 1130)]], [[(980, 985), (1115, 1120)]], [[(995, 1000), (1100, 1105)]], [[(1000, 1003), (1097, 1100)]],
              [[(990, 1000), (1000, 1010), (1090, 1100), (1100, 1110)]]]
    cases.append(("bookended", book_l, [[[(1000, 1100, +1)]], [[(1000, 1100, -1)]]], ((4, 2, 10), (7, 20, 1))))
    # fs = 0 and fe = 2^32 - 1 with F = 2^31: fs - F is negative, fe + F passes 2^32, (x - fs) * Bb passes 2^41.  With flank bins
    # of 2^31 bases a track holds one feature (K_t * w < 2^32)
    far_l = [[[(0, TOP)], []], [[(5, 10), (2 ** 31 - 3, 2 ** 31 + 3), (TOP - 1, TOP)], [(TOP - 9, TOP)]], [[(0, 1)], [(2 ** 31, 2 ** 31 + 1)]]]
    for sigma, name in ((+1, "plus"), (-1, "minus")):
        far_f = [[[(0, TOP, sigma)], []], [[(0, 7, sigma)], []], [[], [(TOP - 4, TOP, sigma)]]]
        cases.append(("far-%s" % name, far_l, far_f, ((1, 1, 2 ** 31), (3, 1, 2 ** 31), (1022, 1, 2 ** 31))))
    far_many = [[[(0, 6, +1), (0, TOP, -1), (2 ** 31, TOP, +1)], [(TOP - 4, TOP, -1)]], [[(1, TOP - 1, +1)], [(0, 1, -1), (0, 2 ** 31, +1)]]]
    cases.append(("far-many", far_l, far_many, ((1000, 12, 2 ** 27), (2, 511, 2 ** 22))))
    return cases
