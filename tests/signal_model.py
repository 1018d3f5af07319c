"""The model of k_signal (gat_amd/csrc/gat_signal.h; include/gat_mi355.h has the definition).  TEST INFRASTRUCTURE ONLY.

A signal track on one group is K >= 0 pieces (s_k, e_k) -- normalized: sorted, disjoint, none empty, adjacent ones allowed --
with a signed integer q_k each.  A segment [s, e) with e > s has c = sum_k |[s, e) n [s_k, e_k)| bases that carry a value and
w = sum_k q_k * |[s, e) n [s_k, e_k)|.  A list of segments adds to four integers: n (segments with e > s), covered (sum of c),
hit (segments with c > 0), sum (of w); segments with e <= s are skipped.  Plain loops over the pieces in Python integers: no
prefix sums, no search.
"""
import numpy as np

WORDS = ("n", "covered", "hit", "sum")
Q_MAX = 2 ** 31 - 1


def _pairs(x):
    """a list of (start, end) Python-integer pairs of a list of pairs or of a structured array with those fields"""
    if isinstance(x, np.ndarray) and x.dtype.names:
        return list(zip(x["start"].tolist(), x["end"].tolist()))
    return [(int(a), int(b)) for a, b in x]


def segment(s, e, pieces, values):
    """(c, w) of the segment [s, e), e > s"""
    c = w = 0
    for (a, b), q in zip(pieces, values):
        ov = min(e, b) - max(s, a)
        if ov > 0:
            c += ov
            w += int(q) * ov
    return c, w


def words(lst, pieces, values):
    """[n, covered, hit, sum] of the segments `lst` against one group's pieces and their values"""
    pieces = _pairs(pieces)
    values = [int(v) for v in values]
    assert len(pieces) == len(values)
    n = covered = hit = total = 0
    for s, e in _pairs(lst):
        if e <= s:
            continue
        c, w = segment(s, e, pieces, values)
        n += 1
        covered += c
        hit += 1 if c > 0 else 0
        total += w
    return [n, covered, hit, total]


def pair_words(segments, track):
    """... of the groups of one segment list and one track: segments[g], track[g] = (pieces, values), summed over the groups"""
    out = [0, 0, 0, 0]
    for seg, (pieces, values) in zip(segments, track):
        out = [a + b for a, b in zip(out, words(seg, pieces, values))]
    assert all(abs(x) < 2 ** 63 for x in out)
    return out


def all_words(lists, tracks):
    """int64 [n_lists, n_tracks, 4]: lists[l][g], tracks[t][g] = (pieces, values)"""
    out = np.zeros((len(lists), len(tracks), len(WORDS)), dtype=np.int64)
    for l, segs in enumerate(lists):
        for t, track in enumerate(tracks):
            out[l, t] = pair_words(segs, track)
    return out


def from_sample(seg, off, n_contigs, tracks):
    """... of Problem.sample's (seg, off) -- sample i's list of contig c at off[i * n_contigs + c] -- against tracks[t][c]"""
    n_samples = (len(off) - 1) // n_contigs if n_contigs else 0
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n_samples)]
    return all_words(lists, tracks)


def is_normalized(t):
    p = _pairs(t)
    return all(b > a for a, b in p) and all(p[i + 1][0] >= p[i][1] for i in range(len(p) - 1))


# ---- the hand cases: (name, segments, pieces, values, [n, covered, hit, sum]) ------------------------------------------------------
P3 = [(100, 200), (300, 400), (400, 450)]                       # (a gap, then two adjacent pieces)
V3 = [5, -2, 7]
LONG = 2 ** 32 - 1
HAND = [
    ("a segment inside one piece", [(120, 130)], P3, V3, [1, 10, 1, 50]),
    ("a segment equal to a piece", [(300, 400)], P3, V3, [1, 100, 1, -200]),
    ("a segment across a gap", [(150, 320)], P3, V3, [1, 70, 1, 50 * 5 - 20 * 2]),
    ("a segment across everything", [(0, 1000)], P3, V3, [1, 250, 1, 500 - 200 + 350]),
    ("adjacent pieces of opposite sign that cancel", [(390, 410)], [(300, 400), (400, 450)], [3, -3], [1, 20, 1, 0]),
    ("bookended on the left of a piece: no hit", [(50, 100)], P3, V3, [1, 0, 0, 0]),
    ("bookended on the right of a piece: no hit", [(200, 300)], P3, V3, [1, 0, 0, 0]),
    ("behind the last piece", [(450, 460)], P3, V3, [1, 0, 0, 0]),
    ("a one-base overlap at the start", [(50, 101)], P3, V3, [1, 1, 1, 5]),
    ("a one-base overlap at the end", [(449, 500)], P3, V3, [1, 1, 1, 7]),
    ("one base on either side of a seam", [(399, 401)], P3, V3, [1, 2, 1, 5]),
    ("segments of no length are skipped", [(120, 120), (130, 120), (120, 130)], P3, V3, [1, 10, 1, 50]),
    ("no pieces", [(10, 20), (5, 5), (30, 31)], [], [], [2, 0, 0, 0]),
    ("pieces of value 0 are covered and hit", [(0, 50)], [(10, 20), (30, 40)], [0, 0], [1, 20, 1, 0]),
    ("unsorted, overlapping segments count on their own", [(500, 600), (120, 130), (0, 1000), (120, 130)], P3, V3, [4, 270, 3, 750]),
    ("the largest value over a long piece", [(0, 2 ** 31), (2 ** 31, LONG)], [(0, LONG)], [Q_MAX], [2, LONG, 2, Q_MAX * LONG]),
    ("the most negative value over a long piece", [(5, 2 ** 31 + 5)], [(0, 2 ** 31), (2 ** 31, LONG)], [-Q_MAX, -Q_MAX],
     [1, 2 ** 31, 1, -Q_MAX * 2 ** 31]),
    ("coordinates at 2^32 - 1", [(LONG - 1, LONG), (0, 1)], [(0, 1), (LONG - 1, LONG)], [-4, 9], [2, 2, 2, 5]),
]
assert any(abs(h[4][3]) > 2 ** 32 for h in HAND) and any(h[4][3] < 0 for h in HAND)


def random_pieces(r, k, span, max_len=12, adjacent=0.3, lo=-5, hi=5):
    """(pieces, values): k sorted, disjoint, non-empty pieces of 1..max_len bases, three in ten neighbours adjacent, with
    values drawn from [lo, hi] (r: random.Random)"""
    out, pos = [], r.randint(0, 20)
    for _ in range(k):
        ln = r.randint(1, max_len)
        out.append((pos, pos + ln))
        pos += ln + (0 if r.random() < adjacent else r.randint(1, max(2, span // max(1, k))))
    return out, [r.randint(lo, hi) for _ in range(k)]


def random_segments(r, n, top, max_len=60, empty=0.1):
    """n arbitrary segments below about `top`: any order, overlapping, one in ten of no length"""
    out = []
    for _ in range(n):
        s = r.randint(0, max(1, top))
        out.append((s, s if r.random() < empty else s + r.randint(1, max_len)))
    return out


def random_normalized(r, k, span, max_len=40):
    """k sorted, disjoint, non-empty segments"""
    return random_pieces(r, k, span, max_len)[0]
