"""Problems at both ends of the coordinate range for the samplers that draw lengths (SamplerAnnotator, SamplerSegments,
SamplerBruteForce) and the helpers their tests share.  TEST INFRASTRUCTURE ONLY.

The placement domain: a segment of `length` bases placed on the workspace piece [cs, ce) starts at
ce - 1 at the latest and so ends at ce + length - 1 at the most; with Lmax the longest length the unit's histogram can
return, `last workspace end + Lmax - 1 <= T = 2^31 - 1` keeps every end a coordinate.  The cases here sit exactly AT that
border (`border(lmax)` is the highest last workspace end), at coordinate 0, or span the whole range between; `past_border`
moves each of them up until its highest possible end is T + 1 (one base, for the cases at the border), where
gat_problem_create must refuse.

A case is a list of units (segments, workspace) -- one contig per unit, no isochores -- a bucket size, a call seed, a
number of samples and one annotation track whose last interval ends at T.  tests/test_range_cases_model.py asserts
every case's premise on the oracle (a case that stops exercising its edge fails there, without a device);
tests/test_coordinate_range_gpu.py runs them on every kernel route; tests/golden/make_goldens_coordinate_range.py records the
reference's own lists for some of them.  nbuckets stays at its default everywhere: the oracle's cost grows with it.
"""
import collections
import functools
import json
import os

import numpy as np

import brute_force_model as BM
import sampler_edges as E
from oracle import oracle as O

T = 2 ** 31 - 1
ANNOTATOR, SEGMENTS, SHIFT, BRUTE = 0, 1, 2, 5
SAMPLER_NAMES = {ANNOTATOR: "annotator", SEGMENTS: "segments", BRUTE: "brute_force"}
NBUCKETS = 100000
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coordinate_range.json")

Case = collections.namedtuple("Case", "name units bucket_size seed samples annos")


# ------------------------------------------------------------------------------------------------ the domain
def bucket_of(segs, ws, bucket_size):
    """getLengthDistribution's bucket (gat/SegmentList.pyx:1148-1184) of the unit's working segments."""
    working = O.aslist(O.filter(segs, ws))
    return bucket_size or -(-max(e - s for s, e in working) // NBUCKETS)


def lmax_of(segs, ws, bucket_size):
    """the longest length HistogramSampler.sample (gat/Engine.pyx:413-435) can return for the unit: randint(1, total) never
    returns `total`, so of two or more working segments the longest one's rank is never drawn -- the second longest
    one's bucket times the bucket size, plus the largest draw inside the bucket when the bucket is above 1."""
    lens = sorted(e - s for s, e in O.aslist(O.filter(segs, ws)))
    bucket = bucket_of(segs, ws, bucket_size)
    top = lens[-2] if len(lens) > 1 else lens[0]
    return -(-top // bucket) * bucket + (bucket - 1 if bucket > 1 else 0)


def border(lmax):
    """the highest end a unit's last workspace piece can have: end + lmax - 1 == T."""
    return T - lmax + 1


def highest_end(case):
    """the largest end a placement of any unit of the case can have."""
    return max(ws[-1][1] + lmax_of(segs, ws, case.bucket_size) - 1 for segs, ws in case.units)


def flat_of(case, sampler, with_annos=True):
    """the flat problem of a case under a sampler kind."""
    flat = E.units_flat(case.units, sampler)
    flat.update(bucket_size=case.bucket_size, nbuckets=NBUCKETS)
    if sampler == BRUTE:
        flat.update(brute_ntries_inner=0, brute_ntries_outer=0)
    if sampler == SHIFT:
        flat.update(shift_radius=2.0, shift_extension=0)
    if with_annos and case.annos is not None:
        assert len(case.annos) == int(flat["n_contigs"])
        flat["n_tracks"] = 1
        flat["annos"] = O.segs([x for a in case.annos for x in a])
        flat["anno_off"] = np.concatenate([[0], np.cumsum([len(a) for a in case.annos])]).astype(np.int64)
    return flat


def moved(case, by, name=None):
    """the case with every coordinate moved up by `by` bases."""
    def mv(lst):
        return [(s + by, e + by) for s, e in lst]
    return case._replace(name=name or "%s+%d" % (case.name, by), units=[(mv(s), mv(w)) for s, w in case.units],
                         annos=None if case.annos is None else [[(s, e) for s, e in mv(a) if e <= T] for a in case.annos])


# ------------------------------------------------------------------------------------------------ the cases
def top_tiny(bucket_size=1, last=None):
    """the border workspace [(T-60, T-20), (T-4, T-3)] and four segments of 4 bases, 128 samples, seed 0: placements on the
    one-base piece at its last offset end exactly at T.  bucket_size 3: lengths of up to 8 are drawn and everything lies
    4 bases lower.  last: another last piece (past the border: the refusal)."""
    lmax = 4 if bucket_size == 1 else -(-4 // bucket_size) * bucket_size + bucket_size - 1
    d = lmax - 4
    segs = [(T - 58 - d + 8 * i, T - 54 - d + 8 * i) for i in range(4)]
    ws = [(T - 60 - d, T - 20 - d), last or (T - 4 - d, T - 3 - d)]
    annos = [[(T - 50, T - 30), (T - 10, T)]]
    return Case("top_tiny_b%d" % bucket_size, [(segs, ws)], bucket_size, 0, 128, annos)


def bottom(first=(5, 3000)):
    """the first piece starts at 5 (or is (0, 1)): 40 segments of 90 bases, placements with q <= 0 start at 0 -- the clamp."""
    ws = [first, (3500, 9000)]
    n_first = 14 if first[1] - first[0] > 90 else 1
    segs = [(first[0] + 5 * (n_first > 1) + 200 * i, first[0] + 5 * (n_first > 1) + 200 * i + 90) for i in range(n_first)]
    step = 200 if n_first > 1 else 135
    segs += [(3600 + step * i, 3690 + step * i) for i in range(40 - n_first)]
    name = "bottom" if first == (5, 3000) else "bottom_%d_%d" % first
    return Case(name, [(segs, ws)], 1, 0, 64, None)


def bottom_brute():
    """`bottom` for SamplerBruteForce, which must place segments.sum() bases exactly and without overlaps -- 40 segments
    of 90 do not converge in `bottom`'s workspace, and a list that holds a clamped segment (overlap below its length) only
    converges where one-base segments can fill up the rest: 6 segments of 8 bases and 12 of one base in [(5, 25), (60, 400)]."""
    segs = [(10 + 3 * i, 11 + 3 * i) for i in range(4)] + [(70 + 20 * i, 78 + 20 * i) for i in range(6)]
    segs += [(200 + 3 * i, 201 + 3 * i) for i in range(8)]
    return Case("bottom_brute", [(segs, [(5, 25), (60, 400)])], 1, 0, 64, None)


def wide_span():
    """two pieces of 2^20 bases, one at 5 and one ending at the border, 60 segments of about 4 000: a sampled list spans
    nearly the whole range (the bucket-sort scale of k_consolidate / k_merge_big, the position grid's top >> shift)."""
    lens = [3900 + 7 * i for i in range(30)]
    lmax = sorted(lens + lens)[-2]
    b = border(lmax)
    lo, hi = (5, 5 + 2 ** 20), (b - 2 ** 20, b)
    segs = [(lo[0] + 100 + 30000 * i, lo[0] + 100 + 30000 * i + lens[i]) for i in range(30)]
    segs += [(hi[0] + 100 + 30000 * i, hi[0] + 100 + 30000 * i + lens[i]) for i in range(30)]
    annos = [[(100, 5000), (2 ** 20, 2 ** 20 + 10), (b - 2 ** 19, T)]]
    return Case("wide_span", [(segs, [lo, hi])], 1, 0, 64, annos)


def _long_segments():
    """30 segments of 2^23 .. 2^24 bases, 35 Mb apart (they fit a piece of 2^30 bases); the two longest are equal, so the
    longest length is one the histogram can draw"""
    return [(10 + 35000000 * i, 10 + 35000000 * i + 2 ** 23 + (2 ** 23 * min(i, 28)) // 28) for i in range(30)]


def whole_range():
    """one piece (0, border), 30 segments of 2^23 .. 2^24 bases, bucket_size 0 (the bucket becomes 168 and Lmax exceeds
    the longest segment): ws_total just under 2^31, position and offset draws under mask 0x7fffffff with almost no
    rejection."""
    segs = _long_segments()
    b = border(lmax_of(segs, [(0, T)], 0))
    return Case("whole_range", [(segs, [(0, b)])], 0, 0, 64, None)


def half_range():
    """the same segments in one piece (3, 2^30 + 5): ws_total just over 2^30, every position and offset draw is rejected
    about every second time, so streams run out of precomputed rows where whole_range's do not."""
    return Case("half_range", [(_long_segments(), [(3, 2 ** 30 + 5)])], 0, 0, 64, None)


def frag_top():
    """300 pieces (more than kPlaceWsLds = 256) of 25 bases, 10 apart, the last ending at the border; 12 segments of 130: a
    placed segment spans several pieces (k_place_grid, the cdf grid and position grid in k_tail, the trees)."""
    b = border(130)
    ws = [(b - 25 - 35 * (299 - k), b - 35 * (299 - k)) for k in range(300)]
    segs = [(ws[0][0] + 3 + 800 * i, ws[0][0] + 133 + 800 * i) for i in range(12)]
    return Case("frag_top", [(segs, ws)], 1, 0, 64, None)


def long_list_top():
    """one unit of 1 200 segments of 40-48 bases in (T - 400 000, border), 64 samples: k_merge_big, k_tail_big,
    k_resume_big."""
    b = border(48)
    segs = [(T - 400000 + 10 + 300 * i, T - 400000 + 10 + 300 * i + 40 + i % 9) for i in range(1200)]
    return Case("long_list_top", [(segs, [(T - 400000, b)])], 1, 0, 64, None)


def top_simple(width=3000):
    """ONE piece of `width` bases ending at the border and 12 segments of 30-41 bases, bucket 1: a "simple" unit, whose
    placement step in k_place / k_place_pipe is the one written out by hand where the offset draw's mask does not depend
    on the length (width 3000: no power of two in (3000, 3041]) and the general step where it does (width 2040: 2048)."""
    lens = [30 + i for i in range(12)]
    b = border(sorted(lens)[-2])
    segs = [(b - width + 10 + 60 * i, b - width + 10 + 60 * i + lens[i]) for i in range(12)]
    return Case("top_simple_%d" % width, [(segs, [(b - width, b)])], 1, 0, 128, None)


# The call seeds of the (case, sampler) pairs whose premise is a rare event (found on the oracle: find_seed); every other pair
# runs under seed 0.  top_tiny under bucket 3: an end at T needs the one-base piece, its last offset and the longest draw --
# one placement in a thousand; bottom_0_1: a start at 0 needs the one-base piece, one base in 5 500; top_simple: the
# piece's last offset, one in 3 000.
SEEDS = {("top_tiny_b3", ANNOTATOR): 384, ("top_tiny_b3", SEGMENTS): 384, ("bottom_0_1", SEGMENTS): 64,
         ("top_simple_3000", ANNOTATOR): 768, ("top_simple_3000", SEGMENTS): 768,
         ("top_simple_2040", ANNOTATOR): 2816, ("top_simple_2040", SEGMENTS): 2816}


def for_sampler(case, sampler):
    """the case under the call seed of the (case, sampler) pair."""
    return case._replace(seed=SEEDS.get((case.name, sampler), case.seed))


def in_domain():
    """every in-domain case, by name."""
    cases = [top_tiny(1), top_tiny(3), bottom(), bottom((0, 1)), bottom_brute(), wide_span(), whole_range(), half_range(),
             frag_top(), long_list_top(), top_simple(3000), top_simple(2040)]
    return collections.OrderedDict((c.name, _with_track(c)) for c in cases)


def _with_track(case):
    """a case that brings no annotation track gets one per unit: the first 50 bases of its workspace, 60 bases near its end,
    and everything from 20 bases before its end up to T."""
    if case.annos is not None:
        return case
    return case._replace(annos=[[(ws[0][0], ws[0][0] + 50), (ws[-1][1] - 100, ws[-1][1] - 40), (ws[-1][1] - 20, T)]
                                for _, ws in case.units])


def past_border():
    """every case above one base further up (the cases that do not lie at the border -- bottom*, half_range: as far up as
    puts their highest end at T + 1), and
    top_tiny with its last piece at (T - 1, T): for the refusal only."""
    cases = [moved(c, T - highest_end(c) + 1) for c in in_domain().values()]
    cases.append(top_tiny(1, last=(T - 1, T))._replace(name="top_tiny_last_piece_at_T"))
    return collections.OrderedDict((c.name, c) for c in cases)


# ------------------------------------------------------------------------------------------------ the oracle's side
COUNTERS = E.ALL_COUNTERS


def oracle_units(case, sampler):
    """(lists, n_draws): the oracle's (sample, unit) lists of the case's call in gat_sample_units' order, and the raw
    MT19937 outputs the call consumed.  SamplerBruteForce: tests/brute_force_model.py."""
    n = len(case.units)
    lists, draws = [], 0
    for s in range(case.samples):
        for u, (segs, ws) in enumerate(case.units):
            rng = O.RandomState((case.seed + s * n + u) & 0xFFFFFFFF)
            if sampler == ANNOTATOR:
                got = O.aslist(O.sampler_annotator(rng, segs, ws, case.bucket_size, NBUCKETS)[0])
            elif sampler == SEGMENTS:
                got = O.aslist(O.sampler_segments(rng, segs, ws, case.bucket_size, NBUCKETS))
            else:
                got = BM.sample(rng, segs, ws, bucket_size=case.bucket_size, nbuckets=NBUCKETS)
            lists.append(got)
            draws += rng.ndraws
    return lists, draws


@functools.lru_cache(maxsize=None)
def oracle_of(name, sampler):
    """oracle_units of the in-domain case `name` under the (case, sampler) pair's call seed: computed once per process,
    shared by the tests and left unchanged by them."""
    return oracle_units(for_sampler(in_domain()[name], sampler), sampler)


@functools.lru_cache(maxsize=None)
def oracle_counts_of(name, sampler):
    """the six counters of the case's annotation track over oracle_of's lists (computed once per process)."""
    return oracle_counts(for_sampler(in_domain()[name], sampler), sampler, oracle_of(name, sampler)[0])


def oracle_counts(case, sampler, lists):
    """the six counters of the case's annotation track over the oracle's lists."""
    return E.model_counts(flat_of(case, sampler), lists, COUNTERS, case.samples)


def ends_at_T(lists):
    """(segments ending exactly at T, segments ending above it)."""
    ends = [e for l in lists for _, e in l]
    return sum(e == T for e in ends), sum(e > T for e in ends)


def starts_at_0(lists):
    return sum(s == 0 for l in lists for s, _ in l)


def widest_list(lists):
    return max((max(e for _, e in l) - min(s for s, _ in l)) for l in lists if l)


def segments_step_draws(case):
    """SamplerSegments replayed step by step on the oracle's generator (HistogramSampler.sample, then
    SegmentListSampler.sample, len(segments) times: gat/Engine.pyx:695-737): (placements, draws of the length steps, draws
    of the placement steps -- the position in the workspace and the offset in the piece), summed over the case's call.
    The replayed lists are the oracle's (asserted)."""
    placements = length_draws = place_draws = 0
    want, _ = oracle_units(case, SEGMENTS)
    n = len(case.units)
    for s in range(case.samples):
        for u, (segs, ws) in enumerate(case.units):
            rng = O.RandomState((case.seed + s * n + u) & 0xFFFFFFFF)
            working = O.aslist(O.filter(segs, ws))
            hist, bucket = O.length_distribution(working, case.bucket_size, NBUCKETS)
            hs = BM.HistogramSampler(hist, bucket)
            cdf, total = [], 0
            for a, b in ws:
                total += b - a
                cdf.append(total - 1)
            got = []
            for _ in range(len(segs)):
                d0 = rng.ndraws
                length = hs.sample(rng)
                d1 = rng.ndraws
                start, end, _ov = BM.sls_sample(rng, ws, cdf, total, length)
                got.append((start, end))
                placements += 1
                length_draws += d1 - d0
                place_draws += rng.ndraws - d1
            assert got == want[s * n + u]
    return placements, length_draws, place_draws


def find_seed(case, premise, sampler, first=0, n=200):
    """the first call seed, from `first` in steps of the call's streams (the stream of (sample s, unit u) is seed + s *
    n_units + u: call seeds closer together share streams), under which premise(lists) holds for the sampler (how SEEDS
    was made)."""
    step = case.samples * len(case.units)
    for seed in range(first, first + n * step, step):
        try:
            if premise(oracle_units(case._replace(seed=seed), sampler)[0]):
                return seed
        except ValueError:
            continue
    return None


def load_golden():
    """tests/golden/coordinate_range.json (tests/golden/make_goldens_coordinate_range.py): {"in_domain": [{case, sampler,
    bucket_size, segments, workspace, streams: [[seed, the reference's list (flat), the next raw output]]}], "past_border":
    [{case, sampler, bucket_size, segments, workspace, streams (how many), highest_end_minus_T, raised: [[seed, exception,
    file, line, text]]}]}"""
    with open(GOLDEN) as f:
        return json.load(f)
