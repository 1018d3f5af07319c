"""Hand-made geometry for the relative distance tests (tests/test_reldist_model.py says what each case is, on the CPU;
tests/test_reldist_gpu.py runs them on the device).  TEST INFRASTRUCTURE ONLY.  A case is (name, lists[l][g], points[t][g], the
bin counts it runs at): at most 3 groups, 3 tracks and 6 lists."""
import random

TOP = 2 ** 32 - 1
ALL_BINS = (1, 2, 64, 66, 1024)
LENGTHS = (0, 1, 63, 64, 65, 130)


def spread_points(r, n, span):
    """n distinct positions below span, ascending"""
    return sorted(r.sample(range(span), n))


def any_segments(r, n, span, max_len):
    """n segments below span in no order, overlapping ones among them"""
    out = []
    for _ in range(n):
        s = r.randrange(0, span - max_len)
        out.append((s, s + r.randint(1, max_len)))
    return out


def hand_geometry():
    cases = []
    # the header's example
    cases.append(("example", [[[(138, 143)]], [[(150, 151)]], [[(100, 101)]], [[(200, 201)]]], [[[100, 200]]], (10,)))
    # list lengths 0, 1, 63, 64, 65, 130 on group 0 (the lane stride and its tail); points per (track, group) 0, 1, 2, 4, 5, 17
    # (the staging limit of 4 and the block table); group 1: points, and segments in every other list only -- track 1 has its
    # points of group 1 where no list has a segment; group 2: segments, and track 0 without a point; track 2 is empty
    r = random.Random(31)
    span = 2000
    lists = []
    for k, n in enumerate(LENGTHS):
        lists.append([any_segments(r, n, span, 12), any_segments(r, 9, span // 2, 30) if k % 2 else [], any_segments(r, 20, span, 5)])
    points = [[spread_points(r, 17, span), [700], []],
              [spread_points(r, 4, span), [span // 2 + 7 * k for k in range(1, 6)], [300, 1500]],
              [[], [], []]]
    cases.append(("lengths", lists, points, ALL_BINS))
    # one group, five lists (more than a workgroup's four waves, and no multiple of a run of 3), the points 100, 101, 110, 120,
    # 200: a gap of 1 and an even gap of 10
    edge_points = [[[100, 101, 110, 120, 200]], [[110]], [[115, 116]]]
    edges = [[[(100, 101), (200, 201), (110, 111)]],             # m == p_0 (in the gap of 1), m == p_{K-1} (outside), m == an interior point
             [[(115, 116), (114, 117), (105, 107), (119, 120)]],   # the centre of the even gap twice, lengths 1, 2 and 3, the last base of a gap
             [[(50, 50), (60, 40), (10, 20), (300, 400)]],         # two that are skipped (e <= s), outside on the left and on the right
             [[(150, 160), (105, 130), (100, 140), (150, 160), (0, 300)]],   # unsorted, overlapping, one twice
             [[]]]
    cases.append(("edges", edges, edge_points, ALL_BINS))
    # points and segments at 0 and at 2^32 - 1, a gap of 2^32 - 1: 2 d B passes 32 bits
    far = [[[(0, 1), (TOP - 1, TOP), (2 ** 31 - 1, 2 ** 31 + 1), (2 ** 30, 2 ** 30 + 1), (0, TOP)], [(TOP - 5, TOP)]],
           [[(2 ** 22, 2 ** 22 + 1), (3 * 2 ** 30, 3 * 2 ** 30 + 2)], [(0, 2), (2, TOP)]]]
    far_points = [[[0, TOP], [TOP]], [[0, 1, TOP], [0, TOP - 3, TOP]], [[TOP], [0]]]
    cases.append(("far", far, far_points, ALL_BINS))
    return cases
