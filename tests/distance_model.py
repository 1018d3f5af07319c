"""The model of k_distance (gat_amd/csrc/gat_distance.h; include/gat_mi355.h has the definition).  TEST INFRASTRUCTURE ONLY.

T is a normalized list (sorted by start, pairwise disjoint, every interval with end > start; adjacent intervals allowed) of
K >= 1 intervals, Q = [s, e) a query with e > s.  j = the first index with T[j].end > s (K: none).  T[j].start < e: d = 0.
Else d = the smaller of T[j].start - e + 1 (where j < K) and s - T[j - 1].end + 1 (where j > 0) -- `bedtools closest -d`:
bookended intervals are at distance 1.  A list of queries against T adds to four integers: n, sum, near (d <= max_distance),
none (the queries where T is empty); queries with e <= s are skipped.  Plain numpy: one searchsorted on the ends.
"""
import numpy as np

WORDS = ("n", "sum", "near", "none")
SEGMENT_TO_ANNOTATION, ANNOTATION_TO_SEGMENT = 0, 1


def _columns(x):
    """(starts, ends) as int64 arrays of a list of (start, end) pairs or of a structured array with those fields"""
    if isinstance(x, np.ndarray) and x.dtype.names:
        return x["start"].astype(np.int64), x["end"].astype(np.int64)
    a = np.array(list(x), dtype=np.int64).reshape(-1, 2)
    return a[:, 0].copy(), a[:, 1].copy()


def is_normalized(t):
    ts, te = _columns(t)
    return bool(np.all(te > ts) and np.all(ts[1:] >= te[:-1]))


def distances(q, t):
    """d of every query of q with e > s against the normalized, non-empty list t: an int64 array, in q's order"""
    qs, qe = _columns(q)
    ts, te = _columns(t)
    assert len(ts) >= 1 and is_normalized(t)
    keep = qe > qs
    qs, qe = qs[keep], qe[keep]
    K = len(ts)
    j = np.searchsorted(te, qs, side="right")                 # the first end > s
    big = np.int64(1) << 40
    right = np.where(j < K, ts[np.minimum(j, K - 1)] - qe + 1, big)
    left = np.where(j > 0, qs - te[np.maximum(j, 1) - 1] + 1, big)
    hit = (j < K) & (ts[np.minimum(j, K - 1)] < qe)
    return np.where(hit, 0, np.minimum(left, right)).astype(np.int64)


def words(q, t, max_distance):
    """[n, sum, near, none] of the queries q against the list t (one group)"""
    qs, qe = _columns(q)
    valid = int((qe > qs).sum())
    if len(_columns(t)[0]) == 0:
        return [0, 0, 0, valid]
    d = distances(q, t)
    return [valid, int(d.sum()), int((d <= int(max_distance)).sum()), 0]


def pair_words(segments, track, direction, max_distance):
    """... of the groups of one segment list and one track: segments[g] and track[g] per group, summed over the groups;
    direction 0 asks from the segments, 1 from the track's intervals"""
    out = np.zeros(len(WORDS), dtype=np.int64)
    for seg, anno in zip(segments, track):
        q, t = (seg, anno) if direction == SEGMENT_TO_ANNOTATION else (anno, seg)
        out += np.array(words(q, t, max_distance), dtype=np.int64)
    return out


def all_words(lists, tracks, direction, max_distance):
    """int64 [n_lists, n_tracks, 4]: lists[l][g], tracks[t][g]"""
    out = np.zeros((len(lists), len(tracks), len(WORDS)), dtype=np.int64)
    for l, segs in enumerate(lists):
        for t, track in enumerate(tracks):
            out[l, t] = pair_words(segs, track, direction, max_distance)
    return out


def from_sample(seg, off, n_contigs, tracks, direction, max_distance):
    """... of Problem.sample's (seg, off) -- sample i's list of contig c at off[i * n_contigs + c] -- against tracks[t][c]"""
    n_samples = (len(off) - 1) // n_contigs if n_contigs else 0
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n_samples)]
    return all_words(lists, tracks, direction, max_distance)


def brute_force(q, t):
    """the smallest gap over all pairs, O(n m): 0 where the two share a base, else the bases between them + 1"""
    qs, qe = _columns(q)
    ts, te = _columns(t)
    out = []
    for s, e in zip(qs.tolist(), qe.tolist()):
        if e <= s:
            continue
        best = None
        for a, b in zip(ts.tolist(), te.tolist()):
            if a < e and s < b:
                d = 0
            elif a >= e:
                d = a - e + 1
            else:
                d = s - b + 1
            best = d if best is None or d < best else best
        out.append(best)
    return out


# ---- the hand cases: (name, queries, T, the distances of the queries that count) -----------------------------------------------
TOP = 2 ** 32 - 1
T3 = [(100, 200), (300, 400), (400, 450)]                       # (the last two adjacent)
HAND = [
    ("before the first interval", [(10, 20)], T3, [81]),
    ("behind the last interval", [(500, 600)], T3, [51]),
    ("bookended left", [(200, 250)], T3, [1]),
    ("bookended right", [(250, 300)], T3, [1]),
    ("bookended on both sides", [(200, 300)], T3, [1]),
    ("one-base overlap at the start", [(50, 101)], T3, [0]),
    ("one-base overlap at the end", [(199, 260)], T3, [0]),
    ("Q contains a T interval", [(90, 210)], T3, [0]),
    ("Q inside a T interval", [(120, 130)], T3, [0]),
    ("Q equal to a T interval", [(300, 400)], T3, [0]),
    ("an equidistant tie", [(240, 260)], T3, [41]),
    ("nearer on the left", [(230, 260)], T3, [31]),
    ("nearer on the right", [(240, 290)], T3, [11]),
    ("adjacent T intervals, Q over the seam", [(399, 401)], T3, [0]),
    ("adjacent T intervals, Q ending at the seam", [(390, 400)], T3, [0]),
    ("one base, in the gap", [(250, 251)], T3, [50]),
    ("coordinates at 2^32 - 1", [(TOP - 1, TOP), (0, 1), (TOP - 10, TOP - 5)], [(5, 6), (TOP - 5, TOP - 1)], [1, 5, 1]),
    ("the largest distance", [(TOP - 1, TOP)], [(0, 1)], [TOP - 1]),
    ("a zero-length query is skipped", [(250, 250), (10, 20), (20, 10)], T3, [81]),
    ("unsorted, overlapping queries", [(500, 600), (10, 20), (90, 210), (10, 20), (0, 1000)], T3, [51, 81, 0, 81, 0]),
    ("a single interval", [(0, 5), (5, 7), (9, 30), (20, 21)], [(7, 9)], [3, 1, 1, 12]),
]
EMPTY_T = ("an empty T", [(10, 20), (5, 5), (30, 31)], [], [0, 0, 0, 2])      # (the words, not the distances)


def random_normalized(r, k, span, max_len=12, adjacent=0.3):
    """k sorted, disjoint, non-empty intervals of 1..max_len bases, three in ten neighbours adjacent (r: random.Random)"""
    out, pos = [], r.randint(0, 20)
    for _ in range(k):
        ln = r.randint(1, max_len)
        out.append((pos, pos + ln))
        pos += ln + (0 if r.random() < adjacent else r.randint(1, max(2, span // max(1, k))))
    return out


def random_queries(r, n, top, max_len=60, empty=0.1):
    """n arbitrary queries below about `top`: any order, overlapping, one in ten of no length"""
    out = []
    for _ in range(n):
        s = r.randint(0, max(1, top))
        out.append((s, s if r.random() < empty else s + r.randint(1, max_len)))
    return out
