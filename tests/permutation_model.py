"""Plain-Python restatement of the reference's SamplerGlobalPermutation.sample (gat/Engine.pyx:1234-1386) on CPython's
own random.Random, in closed form.  TEST INFRASTRUCTURE ONLY: the GPU tests compare the library's global permutation
sampler with it, and tests/test_permutation_model.py pins it to the reference's own output
(tests/golden/permutation/kat.json).  Because the draws come from CPython's generator, the model also pins the
device's init_by_array seeding and _randbelow rule.

The reference's walk (gap, segment, gap, ... from the linear position `shift` of W, wrapping at W's end, splitting a
segment at the gaps between W's pieces) has a closed form: segment x of the shuffled list covers the linear range
[q_x, q_x + L_x) modulo Wsum, q_x = shift + points[x] + P_x with P_x the lengths before it.  The ranges never overlap
and the whole walk spans less than Wsum from `shift`, so the final normalize() only rotates the list to start at its
lowest coordinate: the pieces at linear positions >= Wsum come first.
"""
import json
import os

from oracle import oracle as O

KAT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "permutation", "kat.json")


def load_kats():
    """tests/golden/permutation/kat.json as dicts: segments, workspace, seed, sample (pairs), next."""
    d = json.load(open(KAT))
    return [dict(segments=[tuple(x) for x in d["shapes"][i][0]], workspace=[tuple(x) for x in d["shapes"][i][1]],
                 seed=seed, sample=list(zip(flat[0::2], flat[1::2])), next=nxt)
            for i, seed, flat, nxt in d["cases"]]


def unit_tables(segments, workspace):
    """what problem creation derives for a unit: the working segments' lengths in list order, W = workspace extended by
    the working segments and merge(0)ed, and free = Wsum - sum(lengths).  None when no segment is working."""
    segments = [tuple(x) for x in segments]
    workspace = [tuple(x) for x in workspace]
    working = O.aslist(O.filter(segments, workspace)) if segments and workspace else []
    if not working:
        return None
    W = [tuple(x) for x in O.aslist(O.merge(sorted(workspace + [tuple(x) for x in working]), 0))]
    lengths = [e - s for s, e in working]
    wsum = sum(e - s for s, e in W)
    return lengths, W, wsum - sum(lengths)


def sample(rng, segments, workspace, stats=None):
    """SamplerGlobalPermutation().sample(segments, workspace) drawing from rng (a random.Random).  stats, when given,
    gathers the segments whose range straddles the wrap (linear position Wsum) and the pieces before and after it."""
    t = unit_tables(segments, workspace)
    if t is None:
        return []
    lengths, W, free = t
    if free < 0:
        raise ValueError("free length %d < 0" % free)
    lengths = list(lengths)
    rng.shuffle(lengths)
    points = sorted(rng.randint(0, free) for _ in lengths)
    shift = rng.randint(0, free)
    cum = [0]
    for s, e in W:
        cum.append(cum[-1] + e - s)
    wsum = cum[-1]
    nw = len(W)
    head, tail = [], []                      # pieces at linear positions >= wsum (after the wrap), and before it
    before = 0
    for x, length in enumerate(lengths):
        q = shift + points[x] + before
        before += length
        p, end = q, q + length
        if stats is not None and p < wsum < end:
            stats["straddles"] = stats.get("straddles", 0) + 1
        while p < end:
            turn, lp = divmod(p, wsum)
            j = _piece(cum, lp)
            stop = min(end, turn * wsum + cum[j + 1])
            piece = (W[j][0] + lp - cum[j], W[j][0] + lp - cum[j] + stop - p)
            (head if turn else tail).append(piece)
            p = stop
        assert j < nw
    if stats is not None:
        stats["head"] = stats.get("head", 0) + len(head)
        stats["tail"] = stats.get("tail", 0) + len(tail)
    return head + tail


def _piece(cum, lp):
    """the W piece j with cum[j] <= lp < cum[j + 1]."""
    lo, hi = 0, len(cum) - 1
    while hi - lo > 1:
        m = (lo + hi) // 2
        if cum[m] <= lp:
            lo = m
        else:
            hi = m
    return lo
