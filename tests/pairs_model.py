"""numpy model of the pair hits (gat_list_pair_hits / gat_sample_pair_enrichment).  TEST INFRASTRUCTURE ONLY.

hit(q, t) of a segment q = [s, e), e > s, and a normalized track: j = the first interval with end > s; a hit iff it exists and
starts below e.  c(L, i, j) = the segments of L (all groups; in any order, overlapping or not; e <= s skipped) that hit track i
and track j.  The P = T (T + 1) / 2 pairs in the order (0,0), (0,1), .., (0,T-1), (1,1), ..; and the five words per pair over
a set of samples: n_pos, sum, sumsq, n_less, n_eq.  Lists are sequences of (start, end) or SEG arrays.
"""
import numpy as np

from local_model import pairs as as_pairs     # a list as an int64 array [n, 2]
from local_model import is_normalized, random_normalized, words  # noqa: F401  (the five words are gat-local's: words(values [S][P], obs [P]))

WORDS = ("n_pos", "sum", "sumsq", "n_less", "n_eq")


def pair_list(T):
    """the pairs in their order: [(i, j)], i <= j"""
    return [(i, j) for i in range(T) for j in range(i, T)]


def hits(L, A):
    """hit(q, A) for every segment of L (False where e <= s): bool [len(L)]"""
    L, A = as_pairs(L), as_pairs(A)
    if len(A) == 0 or len(L) == 0:
        return np.zeros(len(L), dtype=bool)
    j = np.searchsorted(A[:, 1], L[:, 0], side="right")            # the first end beyond s
    start = A[np.minimum(j, len(A) - 1), 0]
    return (L[:, 1] > L[:, 0]) & (j < len(A)) & (start < L[:, 1])


def hit_matrix(per_list, tracks):
    """per_list[g], tracks[t][g] -> bool [segments of the list over all groups][T]"""
    rows = [np.stack([hits(seg, tracks[t][g]) for t in range(len(tracks))], axis=1) if len(tracks) else np.zeros((len(seg), 0), dtype=bool)
            for g, seg in enumerate(per_list)]
    return np.concatenate(rows, axis=0) if rows else np.zeros((0, len(tracks)), dtype=bool)


def counts(per_list, tracks):
    """c(L, i, j) of one list for every pair: int64 [P]"""
    h = hit_matrix(per_list, tracks).astype(np.int64)
    full = h.T @ h
    i, j = np.triu_indices(len(tracks))
    return full[i, j].astype(np.int64)


def all_counts(lists, tracks):
    """lists[l][g], tracks[t][g] -> int64 [n_lists][P]"""
    T = len(tracks)
    out = np.zeros((len(lists), T * (T + 1) // 2), dtype=np.int64)
    for l, per_list in enumerate(lists):
        out[l] = counts(per_list, tracks)
    return out


def from_sample(seg, off, n_contigs, tracks):
    """the counts of every sample of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample),
    tracks[t][c] -> int64 [samples][P]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return all_counts(lists, tracks)


def brute_counts(per_list, tracks):
    """c from the definition: every segment against every interval"""
    T = len(tracks)
    out = []
    hit = [[[e > s and any(a < e and s < b for a, b in tracks[t][g]) for t in range(T)] for s, e in seg] for g, seg in enumerate(per_list)]
    for i, j in pair_list(T):
        out.append(sum(1 for g in hit for h in g if h[i] and h[j]))
    return out


def csr(lists_of_lists):
    """entity-major lists[e][g] -> (SEG array, offsets) as the C ABI takes them"""
    SEG = np.dtype([("start", "<u4"), ("end", "<u4")])
    flat = [as_pairs(a) for per in lists_of_lists for a in per]
    off = np.zeros(len(flat) + 1, dtype=np.int64)
    if flat:
        np.cumsum([len(a) for a in flat], out=off[1:])
    seg = np.zeros(int(off[-1]), dtype=SEG)
    if len(seg):
        allp = np.concatenate(flat, axis=0)
        seg["start"], seg["end"] = allp[:, 0].astype(np.uint32), allp[:, 1].astype(np.uint32)
    return seg, off
