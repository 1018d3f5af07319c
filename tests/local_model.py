"""numpy model of the per-bin overlaps (gat_list_bin_overlaps / gat_sample_bin_enrichment).  TEST INFRASTRUCTURE ONLY.

v(L, A, b) = |L n A n [b * bin, (b + 1) * bin)| for normalized lists L and A of one contig, b < n_bins; and the five words per
(track, bin) over a set of samples: n_pos, sum, sumsq, n_less, n_eq.  Lists are sequences of (start, end) or SEG arrays.
"""
import numpy as np

WORDS = ("n_pos", "sum", "sumsq", "n_less", "n_eq")


def pairs(a):
    """a list as an int64 array [n, 2]"""
    if isinstance(a, np.ndarray) and a.dtype.names:
        return np.stack([a["start"].astype(np.int64), a["end"].astype(np.int64)], axis=1)
    return np.array(list(a), dtype=np.int64).reshape(-1, 2)


def is_normalized(a):
    p = pairs(a)
    return bool((p[:, 1] > p[:, 0]).all() and (p[1:, 0] >= p[:-1, 1]).all())


def intersect(L, A):
    """the pieces of L n A, both normalized: int64 [n, 2]"""
    L, A = pairs(L), pairs(A)
    out = []
    i = j = 0
    while i < len(L) and j < len(A):
        s, e = max(L[i, 0], A[j, 0]), min(L[i, 1], A[j, 1])
        if e > s:
            out.append((s, e))
        if L[i, 1] <= A[j, 1]:
            i += 1
        else:
            j += 1
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def binned(pieces, bin_size, n_bins):
    """bases of disjoint pieces in each of n_bins bins of bin_size: int64 [n_bins]; what lies beyond the last bin is dropped"""
    edges = np.arange(n_bins + 1, dtype=np.int64) * int(bin_size)
    if len(pieces) == 0 or n_bins == 0:
        return np.zeros(n_bins, dtype=np.int64)

    def below(x):                                        # sum over the pieces of min(x, edge), for every edge
        x = np.sort(x)
        run = np.concatenate([[0], np.cumsum(x)])
        k = np.searchsorted(x, edges, side="right")
        return run[k] + edges * (len(x) - k)

    return np.diff(below(pieces[:, 1]) - below(pieces[:, 0]))


def values(L, A, bin_size, n_bins):
    """v(L, A, b) for b < n_bins"""
    return binned(intersect(L, A), bin_size, n_bins)


def all_values(lists, tracks, bin_size, n_bins):
    """lists[l][g], tracks[t][g], n_bins[g] -> int64 [n_lists][n_tracks][sum(n_bins)]"""
    total = int(sum(n_bins))
    out = np.zeros((len(lists), len(tracks), total), dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(n_bins)]).astype(np.int64)
    for l, per_list in enumerate(lists):
        for t, per_track in enumerate(tracks):
            for g, nb in enumerate(n_bins):
                out[l, t, off[g]:off[g + 1]] = values(per_list[g], per_track[g], bin_size, int(nb))
    return out


def words(sample_values, observed):
    """sample_values [samples][tracks][bins] (int64), observed [tracks][bins] -> the five words, int64 [tracks][bins][5] as
    Python-integer sums would give them modulo 2^64 (sumsq of a legal call fits)"""
    v = np.asarray(sample_values, dtype=np.int64)
    obs = np.asarray(observed, dtype=np.int64)
    out = np.zeros(obs.shape + (5,), dtype=np.int64)
    out[..., 0] = (v > 0).sum(axis=0)
    out[..., 1] = v.sum(axis=0)
    out[..., 2] = (v.astype(np.uint64) * v.astype(np.uint64)).sum(axis=0, dtype=np.uint64).view(np.int64)
    out[..., 3] = (v < obs[None]).sum(axis=0)
    out[..., 4] = (v == obs[None]).sum(axis=0)
    return out


def from_sample(seg, off, n_contigs, tracks, bin_size, n_bins):
    """the values of every list of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample), tracks[t][c]
    -> int64 [samples][tracks][sum(n_bins)]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return all_values(lists, tracks, bin_size, n_bins)


def brute_values(L, A, bin_size, n_bins):
    """v by a loop over the bases (tiny coordinates only)"""
    out = [0] * n_bins
    top = max([e for _, e in L] + [e for _, e in A] + [0])
    in_l, in_a = [False] * top, [False] * top
    for s, e in L:
        for x in range(s, e):
            in_l[x] = True
    for s, e in A:
        for x in range(s, e):
            in_a[x] = True
    for x in range(top):
        if in_l[x] and in_a[x] and x // bin_size < n_bins:
            out[x // bin_size] += 1
    return out


def random_normalized(r, n, span, max_len=30):
    """up to n sorted disjoint non-empty intervals below span, adjacent ones among them"""
    out, x = [], r.randrange(0, max(1, span // (n + 1)))
    for _ in range(n):
        ln = r.randint(1, max_len)
        if x + ln > span:
            break
        out.append((x, x + ln))
        x += ln + r.choice([0, 0, 1, r.randrange(0, max(1, 2 * span // (n + 1)))])
    return out
