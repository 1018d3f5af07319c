"""numpy / Python-integer model of the relative distance values (gat_list_reldist / gat_sample_reldist_enrichment).  TEST
INFRASTRUCTURE ONLY.

The points of a (track, group) are p_0 < ... < p_{K-1}.  A segment [s, e), e > s, stands for m = s + (e - s) // 2; with j the
first index with p_j > m (K: none) it is inside iff 1 <= j <= K - 1; then d = min(m - p_{j-1}, p_j - m), gap = p_j - p_{j-1}
and its bin is min(B - 1, 2 d B // gap).  A (list, track) has W = B + 3 values, summed over the groups: the bins, then
area = D 10^6 // (n B B) with n the inside segments, C_b the running sum of the bins and D = sum_b |B C_b - (b + 1) n| (0 where
n == 0), then inside and outside.  one_segment is the definition by a scan over the points in Python integers; values does the
same with searchsorted.  Lists are sequences of (start, end) or SEG arrays; points sequences of positions.
"""
import numpy as np

from local_model import pairs, words  # noqa: F401  (the five words are the same)

EXTRA = 3
AREA_SCALE = 10 ** 6
LIMIT = 2 ** 61         # what no intermediate of the 64-bit route may reach


def one_segment(s, e, points, B):
    """None for a skipped segment (e <= s), "outside", or the bin: the definition, by a scan, in Python integers"""
    s, e, B = int(s), int(e), int(B)
    if e <= s:
        return None
    m = s + (e - s) // 2
    K = len(points)
    j = K
    for k in range(K):
        if int(points[k]) > m:
            j = k
            break
    if not 1 <= j <= K - 1:
        return "outside"
    lo, hi = int(points[j - 1]), int(points[j])
    d, gap = min(m - lo, hi - m), hi - lo
    return min(B - 1, 2 * d * B // gap)


def area_route(D, n, B, seen=None):
    """the area by the 64-bit route of include/gat_mi355.h; seen: a list that takes every intermediate"""
    if n == 0:
        return 0
    M = n * B * B
    r = D * 1000
    t = (r % M) * 1000
    if seen is not None:
        seen.extend([M, r, t])
    return (r // M) * 1000 + t // M


def area_of(hist):
    """the area statistic of a histogram over the bins, both ways: they must agree"""
    B = len(hist)
    n = sum(int(v) for v in hist)
    if n == 0:
        return 0
    C = D = 0
    for b in range(B):
        C += int(hist[b])
        D += abs(B * C - (b + 1) * n)
    direct = D * AREA_SCALE // (n * B * B)
    assert D <= n * B * B and direct == area_route(D, n, B) and direct <= AREA_SCALE
    return direct


def group_counts(L, points, B):
    """(histogram int64 [B], outside) of one list of one group against one track's points there"""
    hist = np.zeros(B, dtype=np.int64)
    p = pairs(L)
    p = p[p[:, 1] > p[:, 0]]
    if len(p) == 0:
        return hist, 0
    P = np.array(list(points), dtype=np.int64)
    K = len(P)
    m = p[:, 0] + (p[:, 1] - p[:, 0]) // 2
    j = np.searchsorted(P, m, side="right")
    inside = (j >= 1) & (j <= K - 1)
    if inside.any():
        mi, ji = m[inside], j[inside]
        lo, hi = P[ji - 1], P[ji]
        d = np.minimum(mi - lo, hi - mi)
        hist += np.bincount(np.minimum(B - 1, 2 * d * B // (hi - lo)), minlength=B)
    return hist, int((~inside).sum())


def values(lists, points, B):
    """lists[l][g], points[t][g] -> int64 [n_lists][n_tracks][B + 3], summed over the groups"""
    B = int(B)
    out = np.zeros((len(lists), len(points), B + EXTRA), dtype=np.int64)
    for l, per_list in enumerate(lists):
        for t, per_track in enumerate(points):
            outside = 0
            for g in range(len(per_track)):
                if len(per_list[g]):
                    h, o = group_counts(per_list[g], per_track[g], B)
                    out[l, t, :B] += h
                    outside += o
            out[l, t, B] = area_of(out[l, t, :B])
            out[l, t, B + 1] = out[l, t, :B].sum()
            out[l, t, B + 2] = outside
    return out


def from_sample(seg, off, n_contigs, points, B):
    """the values of every list of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample),
    points[t][c] -> int64 [samples][tracks][B + 3]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return values(lists, points, B)


def point_arrays(points):
    """points[t][g] -> (positions uint32, offsets int64), track-major, as the library takes them"""
    flat = [x for t in points for x in t]
    off = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    return np.array([a for x in flat for a in x], dtype=np.uint32), off
