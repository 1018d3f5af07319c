"""numpy model of the metagene along scaled features (gat_list_metagene / gat_sample_metagene_enrichment).  TEST INFRASTRUCTURE
ONLY.

A feature is (fs, fe, sigma), sigma +1 or -1, len = fe - fs; Bb body bins, Bf flank bins of w bases, F = Bf * w, B = 2 Bf + Bb.
For a plus feature base x of the window [fs - F, fe + F) lies in bin floor((x - (fs - F)) / w) upstream of fs, in
Bf + floor((x - fs) * Bb / len) in the body, and in Bf + Bb + floor((x - fe) / w) from fe on; a minus feature is the mirror,
bin(x; -) = bin(fs + fe - 1 - x; +).  Here bin b is taken as the interval of BASES it covers -- the B + 1 edges of a feature in
one array, mirrored whole for a minus feature -- and a segment's share of it is the length of their intersection, for all bins
at once: deliberately neither the first / last / whole decomposition of the flanks nor the stepping of the body's edges the
kernel uses.  brute_values is the definition itself, base by base.  Lists are sequences of (start, end) or SEG arrays;
features sequences of (start, end, sigma).
"""
import numpy as np

from local_model import is_normalized, pairs, random_normalized, words  # noqa: F401  (the five words are the same)
from profile_model import finish  # noqa: F401

BASES, MIDPOINTS = 0, 1


def n_bins(Bb, Bf):
    return 2 * int(Bf) + int(Bb)


def bin_of(x, fs, fe, sigma, Bb, Bf, w):
    """the bin of base x along (fs, fe, sigma), None outside the window: the definition, in Python integers"""
    F = Bf * w
    if sigma < 0:
        x = fs + fe - 1 - x
    if not fs - F <= x < fe + F:
        return None
    if x < fs:
        return (x - (fs - F)) // w
    if x < fe:
        return Bf + (x - fs) * Bb // (fe - fs)
    return Bf + Bb + (x - fe) // w


def brute_values(L, features, Bb, Bf, w, mode=BASES):
    """v by a loop over the bases (tiny segments only)"""
    out = [0] * n_bins(Bb, Bf)
    for s, e in pairs(L).tolist():
        if mode == MIDPOINTS:
            s = s + (e - s) // 2
            e = s + 1
        for fs, fe, sigma in features:
            for x in range(s, e):
                b = bin_of(x, fs, fe, sigma, Bb, Bf, w)
                if b is not None:
                    out[b] += 1
    return out


def bin_bases(fs, fe, sigma, Bb, Bf, w):
    """the bases of every bin of one feature: (lo, hi) int64 [B], bin b holding [lo[b], hi[b]) -- empty where lo == hi"""
    fs, fe, Bb, Bf, w = int(fs), int(fe), int(Bb), int(Bf), int(w)
    F, length = Bf * w, fe - fs
    k = np.arange(Bb + 1, dtype=np.int64)
    flank = np.arange(Bf, dtype=np.int64) * w
    # the oriented offsets at which the bins begin, and the end of the last: body bin k begins at ceil(k * len / Bb)
    edges = np.concatenate([flank, F - (-(k * length) // Bb), F + length + w + flank])
    if sigma > 0:
        return fs - F + edges[:-1], fs - F + edges[1:]
    return fe + F - edges[1:], fe + F - edges[:-1]


def values(L, features, Bb, Bf, w, mode=BASES):
    """v(L, features, b) of one group for b < B: int64 [B]"""
    out = np.zeros(n_bins(Bb, Bf), dtype=np.int64)
    p = pairs(L)
    if len(p) == 0:
        return out
    s, e = p[:, 0], p[:, 1]
    if mode == MIDPOINTS:
        s = s + (e - s) // 2
        e = s + 1
    F = int(Bf) * int(w)
    for fs, fe, sigma in features:
        # (only the segments that reach the window: the rest share nothing with any bin)
        near = (e > int(fs) - F) & (s < int(fe) + F)
        if near.any():
            lo, hi = bin_bases(fs, fe, sigma, Bb, Bf, w)
            out += np.clip(np.minimum(e[near, None], hi[None]) - np.maximum(s[near, None], lo[None]), 0, None).sum(axis=0)
    return out


def all_values(lists, features, Bb, Bf, w, mode=BASES):
    """lists[l][g], features[t][g] -> int64 [n_lists][n_tracks][B], summed over the groups"""
    out = np.zeros((len(lists), len(features), n_bins(Bb, Bf)), dtype=np.int64)
    for l, per_list in enumerate(lists):
        for t, per_track in enumerate(features):
            for g in range(len(per_track)):
                if len(per_track[g]) and len(per_list[g]):
                    out[l, t] += values(per_list[g], per_track[g], Bb, Bf, w, mode)
    return out


def from_sample(seg, off, n_contigs, features, Bb, Bf, w, mode=BASES):
    """the values of every list of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample),
    features[t][c] -> int64 [samples][tracks][B]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return all_values(lists, features, Bb, Bf, w, mode)


def bounds(features, Bb, Bf, w):
    """most_t of every track: the larger of K_t * w (with flanks) and sum_f ceil(len_f / Bb), features[t][g]"""
    out = []
    for per_track in features:
        flat = [f for g in per_track for f in g]
        out.append(max(len(flat) * int(w) if Bf > 0 else 0, sum(-(-(fe - fs) // int(Bb)) for fs, fe, _ in flat)))
    return out


def feature_key(f):
    return (f[0], f[1], 1 if f[2] < 0 else 0)


def feature_arrays(features):
    """features[t][g] -> (starts uint32, ends uint32, minus uint8, offsets int64), track-major, as the library takes them"""
    flat = [x for t in features for x in t]
    off = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    fs = np.array([f[0] for x in flat for f in x], dtype=np.uint32)
    fe = np.array([f[1] for x in flat for f in x], dtype=np.uint32)
    minus = np.array([1 if f[2] < 0 else 0 for x in flat for f in x], dtype=np.uint8)
    return fs, fe, minus, off
