"""k_consolidate's sort of 513..1 024 placed segments (wave_sort_bucket_sparse<16, 1024>): the one-unit problems that sit on
its borders, and what the oracle alone says about the lists it is handed.  TEST INFRASTRUCTURE ONLY, no GPU import:
tests/test_consolidate_sort_1024_cases_model.py checks the table on the CPU, tests/test_consolidate_sort_1024_gpu.py runs it.

Every case is one unit, samples [BEGIN, BEGIN + S): two tiles of 64, the second partial.  first_lists() replays the placement
loop (gat/Engine.pyx:572-606) on the oracle's generator up to the first consolidation and returns the list the sort is handed;
occupancy() maps it to the kernel's buckets: lo = the smallest start, 1 024 buckets over the span of the starts, bucket =
umulhi(start - lo, scale) with scale = a float quotient just below 1 024 * 2^32 / span.  The rounding of that quotient is
bracketed (a factor 1 - 2^-19 .. 1 - 2^-21), and a case's figures are only used where both ends of the bracket agree.

The comb: pieces of 8 bases, `pitch` apart, three segments of 2 bases in each of the first pieces.  A placement overlaps its
piece by 1 or 2 bases (16 / 9 on average), so the list at the first consolidation has 9 / 8 of the unit's segments -- +- 8,
where a spread list of n has n +- 15: lengths of 576/577, 960/961 and 1 024 from units the split path still takes (n <= 911),
within the ccap of the class, roundup32(n + n / 12 + 64).  A piece's nine starts lie in one bucket or two, about 1.5 elements a
piece.  A wide LAST piece makes the last bucket -- the one whose base is the list's length less its own count, the largest
base there is -- as full as its width says: the largest start lies in it, and every start of the piece within its width below.

Not built, because the sampler cannot produce them:
  * a list whose fullest bucket holds ONE element: 513 or more independently drawn starts in 1 024 buckets collide with
    probability 1 - exp(-n^2 / 2048), that is 1 - 1e-56 at n = 513;
  * all starts equal: a choice one base wide is a workspace of one base, whose unit has one base to cover and places nothing.
So the sort's `span == 0` return is run by no test, at sixteen rounds as at four and eight (tests/test_consolidate_sort.py leaves
it out for the same reason): it is one statement in front of the first LDS access, shared by the three instantiations.
"""
import collections
import functools

import numpy as np

import brute_force_model as BM
import consolidate_route_cases as K
import rows_cases as RC
from oracle import oracle as O

BEGIN = 1000                 # sample_begin: not 0
S = 70                       # two tiles, the second partial
NB = 1024
BANDS = ((2, 4), (5, 8), (9, 16), (17, 10 ** 9))


def _comb(n, pitch, last=0, lens=(2,), n_pieces=None, seed=5):
    """n segments, three to a piece of 8 bases (at 0, 3, 6; lengths from `lens`, 2 at the most), pieces `pitch` bases apart,
    n_pieces of them (default: 7 / 9 of n, the workspace 3.1 times the segments' bases), then a last piece of `last` bases"""
    rs = np.random.RandomState(seed)
    n_pieces = n_pieces or (n * 7 + 8) // 9
    assert 3 * n_pieces >= n and pitch >= 16 and max(lens) <= 2
    segs = []
    for i in range(n):
        at = 1000 + (i // 3) * pitch + 3 * (i % 3)
        segs.append((at, at + int(lens[rs.randint(len(lens))])))
    ws = [(1000 + k * pitch, 1000 + k * pitch + 8) for k in range(n_pieces)]
    if last:
        at = 1000 + n_pieces * pitch
        ws.append((at, at + last))
    return segs, ws


def _case(name, unit, spread=False):
    return K._case(name, "s", unit, S, spread=spread)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [
        # ---- size borders
        _case("s_spread500", K._spread(500, 2500), spread=True),       # placed counts on both sides of 512 | 513
        _case("s_spread520", K._spread(520, 2520), spread=True),
        _case("s_576", _comb(512, 112)),                               # 9 / 8 of 512 = 576: a round of 64 ends there
        _case("s_960", _comb(855, 112)),                               # 961.9: the fifteenth round ends at 960
        _case("s_911", K._spread(911, 2911), spread=True),             # the largest unit of the split path
        _case("s_1024", _comb(910, 112)),                              # 1 023.75; beyond 1 024 the list is wave_sort_bucket_global's
        # ---- occupancy bands (the last bucket: about 0.18 elements a base of the last piece; the pitch keeps a bucket wider than it)
        _case("o_plain", _comb(600, 112)),                             # 2-4 and 5-8
        _case("o_last12", _comb(600, 200, last=66)),                   # 9-16
        _case("o_last16", _comb(600, 260, last=94)),                   # around 16 | 17: sparse sort and network
        _case("o_last27", _comb(600, 400, last=150)),                  # 17 or more: the network
        # ---- the 10-bit base: 1 000 elements and more, the last bucket crowded
        _case("b_base1000", _comb(903, 130, last=66)),
        # ---- ties: equal starts, ends that differ (lengths 1 and 2)
        _case("t_ties", _comb(640, 112, lens=(1, 2))),
    ]
    return collections.OrderedDict((c.name, c) for c in cs)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(flat, counts, (segments, offsets)) of the oracle for samples [BEGIN, BEGIN + S): once per case, shared, read-only"""
    case = cases()[name]
    flat = K.flat_of(case)
    want, wsamples = O.run_samples(flat, list(case.counters), K.SEED, 1, BEGIN, BEGIN + S, want_samples=True)
    for a in list(want) + list(wsamples):
        a.setflags(write=False)
    return flat, want, wsamples


@functools.lru_cache(maxsize=None)
def first_lists(name):
    """per sample: the placed segments, in placement order, when the loop first consolidates (K.placed_counts with the list)"""
    (segs, ws), = cases()[name].units
    ws = [tuple(x) for x in ws]
    work = O.aslist(O.filter(segs, ws))
    hist, bucket = O.length_distribution(work, 1, K.NBUCKETS)
    hs = BM.HistogramSampler(hist, bucket)
    ltotal = O.total(O.intersect(work, ws))
    cdf, total = [], 0
    for a, b in ws:
        total += b - a
        cdf.append(total - 1)
    out = []
    for s in range(BEGIN, BEGIN + S):
        rng = O.RandomState((K.SEED + s) & 0xFFFFFFFF)
        remaining, lst = ltotal, []
        while True:
            length = hs.sample(rng)
            if remaining <= length:
                break
            start, end, ov = BM.sls_sample(rng, ws, cdf, total, length)
            lst.append((start, end))
            remaining -= ov
        out.append(tuple(lst))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def stream_stats(name):
    """(n_placed, n_draws, n_unsuccessful) of the case's call from the full replay of every stream, which must give the oracle's lists"""
    (segs, ws), = cases()[name].units
    _, _, (seg, off) = reference(name)
    placed = draws = nuns = 0
    for i, s in enumerate(range(BEGIN, BEGIN + S)):
        r = RC.replay_annotator((K.SEED + s) & 0xFFFFFFFF, segs, ws, 1)
        assert r[0] == O.aslist(seg[off[i]:off[i + 1]]), (name, s)
        assert r[6] == len(first_lists(name)[i]), (name, s)
        placed += r[4]
        draws += r[3]
        nuns += r[2]
    return placed, draws, nuns


def _buckets(starts, factor):
    lo, hi = min(starts), max(starts)
    span = hi - lo
    if span == 0:
        return None
    if span < NB:
        return [s - lo for s in starts]
    scale = int((NB << 32) / span * factor)
    return [((s - lo) * scale) >> 32 for s in starts]


Occupancy = collections.namedtuple("Occupancy", "n fullest last_count last_base collided ties")


@functools.lru_cache(maxsize=None)
def occupancy(name):
    """per sample an Occupancy, or None where the two ends of the scale's bracket disagree about any of it: n = the list's
    length, fullest = its fullest bucket, last_count / last_base = the members of the bucket of the largest start and the
    elements in front of it, collided = buckets of two or more, ties = pairs of equal starts with different ends in a bucket"""
    out = []
    for lst in first_lists(name):
        starts = [s for s, _ in lst]
        res = []
        for factor in (1.0 - 2.0 ** -19, 1.0 - 2.0 ** -21):
            b = _buckets(starts, factor)
            cnt = collections.Counter(b)
            last = max(b)
            by_start = collections.defaultdict(set)
            for (s, e) in lst:
                by_start[s].add(e)
            res.append(Occupancy(len(lst), max(cnt.values()), cnt[last], len(lst) - cnt[last], sum(1 for c in cnt.values() if c >= 2),
                                 sum(len(v) - 1 for v in by_start.values())))
        out.append(res[0] if res[0] == res[1] else None)
    return tuple(out)


def band_of(fullest):
    for lo, hi in BANDS:
        if lo <= fullest <= hi:
            return (lo, hi)
    return None
