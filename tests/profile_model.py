"""numpy model of the profile around anchors (gat_list_profile / gat_sample_profile_enrichment).  TEST INFRASTRUCTURE ONLY.

An anchor is (a, sigma), sigma +1 or -1; w = bin_size, H = half_bins, R = H * w, B = 2 H.  The offset of base x is
o = sigma * (x - a); x is in the window iff -R <= o < R; its bin is floor((o + R) / w).  Here bin b is taken as the interval of
BASES it covers -- [a - R + b w, a - R + (b + 1) w) for a plus anchor, [a + R - (b + 1) w + 1, a + R - b w + 1) for a minus one
-- and a segment's share of it is the length of their intersection, for all bins at once: deliberately not the first / last /
whole decomposition the kernel uses.  brute_values is the definition itself, base by base.  Lists are sequences of (start,
end) or SEG arrays; anchors sequences of (position, sigma).
"""
import numpy as np

from local_model import is_normalized, pairs, random_normalized, words  # noqa: F401  (the five words are the same)

BASES, MIDPOINTS = 0, 1


def bin_of(x, a, sigma, w, H):
    """the bin of base x around (a, sigma), None outside the window: the definition, in Python integers"""
    o = sigma * (x - a)
    R = H * w
    return (o + R) // w if -R <= o < R else None


def brute_values(L, anchors, w, H, mode=BASES):
    """v by a loop over the bases (tiny segments only)"""
    out = [0] * (2 * H)
    for s, e in pairs(L).tolist():
        if mode == MIDPOINTS:
            s = s + (e - s) // 2
            e = s + 1
        for a, sigma in anchors:
            for x in range(s, e):
                b = bin_of(x, a, sigma, w, H)
                if b is not None:
                    out[b] += 1
    return out


def values(L, anchors, w, H, mode=BASES):
    """v(L, anchors, b) of one group for b < 2 H: int64 [2 H]"""
    w, H = int(w), int(H)
    B, R = 2 * H, H * w
    out = np.zeros(B, dtype=np.int64)
    p = pairs(L)
    if len(p) == 0:
        return out
    s, e = p[:, 0], p[:, 1]
    if mode == MIDPOINTS:
        s = s + (e - s) // 2
        e = s + 1
    b = np.arange(B, dtype=np.int64)
    for a, sigma in anchors:
        a = int(a)
        lo = a - R + b * w if sigma > 0 else a + R - (b + 1) * w + 1
        # (only the segments that reach the window: the rest share nothing with any bin)
        near = (e > a - R) & (s <= a + R)
        if near.any():
            out += np.clip(np.minimum(e[near, None], lo[None] + w) - np.maximum(s[near, None], lo[None]), 0, None).sum(axis=0)
    return out


def all_values(lists, anchors, w, H, mode=BASES):
    """lists[l][g], anchors[t][g] -> int64 [n_lists][n_tracks][2 H], summed over the groups"""
    out = np.zeros((len(lists), len(anchors), 2 * int(H)), dtype=np.int64)
    for l, per_list in enumerate(lists):
        for t, per_track in enumerate(anchors):
            for g in range(len(per_track)):
                if len(per_track[g]) and len(per_list[g]):
                    out[l, t] += values(per_list[g], per_track[g], w, H, mode)
    return out


def from_sample(seg, off, n_contigs, anchors, w, H, mode=BASES):
    """the values of every list of a Problem.sample: seg / off as returned (sample-major, n_contigs lists a sample),
    anchors[t][c] -> int64 [samples][tracks][2 H]"""
    n = (len(off) - 1) // n_contigs
    lists = [[seg[off[i * n_contigs + c]:off[i * n_contigs + c + 1]] for c in range(n_contigs)] for i in range(n)]
    return all_values(lists, anchors, w, H, mode)


def finish(partial, obs, S):
    """k_null_finish: words [.., 5] that count only the samples with v > 0 in n_less / n_eq, completed over S samples"""
    out = np.array(partial, dtype=np.int64, copy=True)
    obs = np.asarray(obs, dtype=np.int64)
    zeros = S - out[..., 0]
    out[..., 3] += zeros * (obs > 0)
    out[..., 4] += zeros * (obs == 0)
    return out


def anchor_arrays(anchors):
    """anchors[t][g] -> (positions uint32, minus uint8, offsets int64), track-major, as the library takes them"""
    flat = [x for t in anchors for x in t]
    off = np.concatenate([[0], np.cumsum([len(x) for x in flat])]).astype(np.int64)
    pos = np.array([a for x in flat for a, _ in x], dtype=np.uint32)
    minus = np.array([1 if sigma < 0 else 0 for x in flat for _, sigma in x], dtype=np.uint8)
    return pos, minus, off
