"""Problems whose streams run out of the rows k_rng generated ahead, at a row count the test chooses, and the oracle's side
of their calls.  TEST INFRASTRUCTURE ONLY.

The row budget of a unit (rng_rows_for_unit, gat_prep.hip) is ceil((e * n * GAT_RNG_SLACK + sigmas * spread +
GAT_RNG_TAIL_ROWS) / 16) * 16.  With GAT_RNG_SLACK=0 and both sigma knobs at 0 it is GAT_RNG_TAIL_ROWS rounded up to 16
for a unit of at most 65 working segments (the sigma multiple is max(s_min, s_min - 0.5 + n / 130) = 0), for a long list
and for SamplerSegments (both take s_max = 0); a unit in between keeps a spread term of a few dozen rows, and a step of 16
in GAT_RNG_TAIL_ROWS is a step of 16 in its rows all the same.  The cases here are problems of ONE unit, so that
Problem.rows_per_sample() IS that unit's row count; tests/test_rows_run_out_gpu.py moves it onto every target of the tables
below and compares what the device samples with the oracle, whose lists do not depend on the budget: one oracle run per
case serves every row count.

What the oracle keeps per (sample, unit) stream, from RandomState((seed + s * n_units + u) mod 2^32): its list, D (raw
MT19937 outputs consumed: rng.ndraws) and nunsuccessful -- and, from a replay of SamplerAnnotator.sample step by step on
the same generator (asserted to give the oracle's list and D), where the stream stood at its first consolidation, how long
its list was at every consolidation, and how many outputs the reference's last, discarded placement took: the device stops
at the consolidation that ends the loop, so a stream needs `used = D - discarded` outputs there.

tests/test_rows_cases_model.py asserts on the oracle alone that every case and table does what it is here for.
"""
import collections
import functools

import numpy as np

import brute_force_model as BM
import sampler_edges as E
from oracle import oracle as O

ANNOTATOR, SEGMENTS = 0, 1
NBUCKETS = 100000
MT_N = 624
SAMPLES = 70                           # two tiles of 64 streams, the second one partial
BEGIN = 3                              # sample_begin of the calls: sample s of a one-unit problem draws from stream seed + s
SEED = 11
COUNTERS = E.ALL_COUNTERS

Case = collections.namedtuple("Case", "name units bucket_size annos isochores")
Stream = collections.namedtuple("Stream", "lst D nuns used placed first_at first_n cons_n")


# ------------------------------------------------------------------------------------------------ the cases
def _unit(n, lens, pieces, step):
    """n segments of lens[i % len(lens)] bases, `step` apart, from 50 bases into the first piece on; a segment that would
    reach into a gap between two pieces moves to the next piece's start + 50."""
    segs, x, k = [], pieces[0][0] + 50, 0
    for i in range(n):
        ln = lens[i % len(lens)]
        while x + ln > pieces[k][1]:
            k += 1
            x = pieces[k][0] + 50
        segs.append((x, x + ln))
        x += step
    return segs, list(pieces)


def _annos(ws):
    """one track: the first 500 bases of the workspace, a stretch in its middle, everything from 300 bases before its end"""
    lo, hi = ws[0][0], ws[-1][1]
    mid = (lo + hi) // 2
    return [(lo, lo + 500), (mid, mid + (hi - lo) // 10), (hi - 300, hi + 1000)]


def _single(name, unit, bucket_size=1):
    return Case(name, [unit], bucket_size, [_annos(unit[1])], False)


def small(bucket_size=1):
    """40 segments of 30-44 bases in three pieces: lists of at most 64 at every consolidation (the insertion sort), and at
    most 65 working segments: rows == GAT_RNG_TAIL_ROWS rounded up to 16, exactly."""
    u = _unit(40, list(range(30, 45)), [(1000, 9000), (10000, 14000), (15000, 40000)], 700)
    return _single("small" if bucket_size == 1 else "small_b%d" % bucket_size, u, bucket_size)


def mid():
    """250 segments of 40-48 bases in three pieces (k_place's general form): lists of 65..512.  Each piece and the workspace are
    just under a power of two long and the histogram holds 250 ranks, so hardly a draw is rejected: the streams' output
    counts lie within 55 of one another, and one row count can end nearly all of them behind their first consolidation."""
    return _single("mid", _unit(250, list(range(40, 49)), [(2000, 67400), (70000, 102700), (110000, 142700)], 500))


def mid_simple():
    """`mid` in ONE piece of 65 400 bases (no power of two in (65400, 65448]): a simple unit whose placement step is the
    one written out by hand; a call of two tiles takes k_place_scan by default, and k_place_wide, k_place_pipe and k_place
    under PLACE_ROUTES."""
    return _single("mid_simple", _unit(250, list(range(40, 49)), [(3000, 68400)], 260))


def mid_grid():
    """172 segments of 40-48 bases in 300 pieces (more than kPlaceWsLds = 256) of 400 bases, 100 apart: k_place_grid."""
    ws = [(1000 + 500 * k, 1400 + 500 * k) for k in range(300)]
    return _single("mid_grid", _unit(172, list(range(40, 49)), ws, 860))


def large():
    """600 segments of 40-48 bases in three pieces of 3 Mb in all: so sparse that the first consolidation comes after
    nearly 600 placements -- a list of 513..1024."""
    return _single("large", _unit(600, list(range(40, 49)), [(5000, 1000000), (1100000, 2000000), (2100000, 3200000)], 4800))


def long():
    """1 100 segments of 40-48 bases: lists beyond 1024 -- k_merge_big, k_tail_big, k_resume_big."""
    return _single("long", _unit(1100, list(range(40, 49)), [(5000, 2000000), (2100000, 4000000), (4100000, 6000000)], 5000))


def multi():
    """four units of different size classes in one problem: an isochore pair (units 0 and 1, one contig: k_contig reads
    resumed units) of 150 and 40 segments, a unit of 300 and one of 12.  Used with GAT_RNG_SLACK only."""
    units = [_unit(150, list(range(40, 49)), [(2000, 60000), (70000, 90000)], 500),
             _unit(40, list(range(30, 45)), [(100000, 140000), (150000, 180000)], 1500),
             _unit(300, list(range(40, 49)), [(1000, 400000), (500000, 900000)], 2500),
             _unit(12, [90, 110, 130], [(500, 9000)], 600)]
    c0 = sorted(units[0][1] + units[1][1])
    annos = [_annos(c0), _annos(units[2][1]), _annos(units[3][1])]
    return Case("multi", units, 1, annos, True)


@functools.lru_cache(maxsize=None)
def cases():
    cs = [small(), small(3), mid(), mid_simple(), mid_grid(), large(), long(), multi()]
    return collections.OrderedDict((c.name, c) for c in cs)


def flat_of(case, sampler, with_annos=True):
    """the flat problem of a case under a sampler kind; `isochores`: units 0 and 1 are the isochores of contig 0."""
    flat = E.units_flat(case.units, sampler)
    flat.update(bucket_size=case.bucket_size, nbuckets=NBUCKETS)
    if case.isochores:
        n = len(case.units)
        flat["unit_contig"] = np.array([0, 0] + list(range(1, n - 1)), dtype=np.int32)
        flat["n_contigs"] = n - 1
        flat["merge_contigs"] = 1
        ws0 = O.aslist(O.normalize(sorted(case.units[0][1] + case.units[1][1])))
        flat["cws_nseg"] = np.array([len(ws0)] + [len(w) for _, w in case.units[2:]], np.int64)
    if with_annos and sampler != SEGMENTS:
        assert len(case.annos) == int(flat["n_contigs"])
        flat["n_tracks"] = 1
        flat["annos"] = O.segs([x for a in case.annos for x in a])
        flat["anno_off"] = np.concatenate([[0], np.cumsum([len(a) for a in case.annos])]).astype(np.int64)
    return flat


# ------------------------------------------------------------------------------------------------ the oracle's side
def replay_annotator(seed, segs, ws, bucket_size):
    """SamplerAnnotator.sample (gat/Engine.pyx:515-646) step by step on the oracle's generator and list operations: (list,
    D, nunsuccessful, used, placed, first_at, first_n, cons_n) -- used: the outputs consumed up to the consolidation that
    ends the loop (everything but the last, discarded placement :628); placed: segments added to `sampled`; first_at: the
    outputs consumed before the length draw in front of the first consolidation (what the placement kernels consume is
    that draw more); first_n and cons_n: the list's length (unintersected + sampled) at the first and at every
    consolidation."""
    rng = O.RandomState(seed)
    working = O.aslist(O.filter(segs, ws))
    ltotal = O.total(O.intersect(working, ws))
    hist, bucket = O.length_distribution(working, bucket_size, NBUCKETS)
    hs = BM.HistogramSampler(hist, bucket)
    cdf, total = [], 0
    for a, b in ws:
        total += b - a
        cdf.append(total - 1)
    remaining = true_remaining = ltotal
    nuns = placed = 0
    sampled, unint = [], O.segs([])
    first_at, cons_n, used = None, [], 0
    while true_remaining > 0 and nuns < 20:
        before = rng.ndraws
        length = hs.sample(rng)
        if remaining <= length:
            if first_at is None:
                first_at = before
            cons_n.append(len(unint) + len(sampled))
            unint = O.merge(sorted(O.aslist(unint) + sampled), 0)
            sampled = []
            remaining = ltotal - O.total(O.intersect(unint, ws))
            if true_remaining == remaining:
                nuns += 1
            else:
                true_remaining = remaining
            used = rng.ndraws
        if true_remaining < 0:
            lst = O.aslist(unint)
            ucdf, utotal = [], 0
            for a, b in lst:
                utotal += b - a
                ucdf.append(utotal - 1)
            start, _end, _ov = BM.sls_sample(rng, lst, ucdf, utotal, 1)
            forward = rng.randint(0, 2)
            unint = O.trim_ends(unint, start, -true_remaining, forward)
            true_remaining = 1
            continue
        start, end, ov = BM.sls_sample(rng, ws, cdf, total, length)
        if true_remaining > 0:
            sampled.append((start, end))
            placed += 1
            remaining -= ov
    out = O.aslist(O.filter(O.merge(unint, 0), ws))
    return out, rng.ndraws, nuns, used, placed, first_at, cons_n[0], cons_n


@functools.lru_cache(maxsize=None)
def streams_of(name, sampler=ANNOTATOR, begin=BEGIN, samples=SAMPLES):
    """the Stream of every (sample, unit) of the case's call (seed SEED, samples [begin, begin + samples)) in
    gat_sample_units' order: computed once per process, shared by the tests and left unchanged by them.  SamplerSegments
    never consolidates: used == D, the other replay fields are None."""
    case = cases()[name]
    n = len(case.units)
    out = []
    for s in range(begin, begin + samples):
        for u, (segs, ws) in enumerate(case.units):
            seed = (SEED + s * n + u) & 0xFFFFFFFF
            rng = O.RandomState(seed)
            if sampler == SEGMENTS:
                lst = O.aslist(O.sampler_segments(rng, segs, ws, case.bucket_size, NBUCKETS))
                out.append(Stream(lst, rng.ndraws, 0, rng.ndraws, len(lst), None, None, None))
                continue
            got, nuns = O.sampler_annotator(rng, segs, ws, case.bucket_size, NBUCKETS)
            lst = O.aslist(got)
            r = replay_annotator(seed, segs, ws, case.bucket_size)
            assert r[0] == lst and r[1] == rng.ndraws and r[2] == nuns, (name, s, u)
            out.append(Stream(lst, rng.ndraws, nuns, *r[3:]))
    return tuple(out)


def lists_of(name, sampler=ANNOTATOR, begin=BEGIN, samples=SAMPLES):
    return [st.lst for st in streams_of(name, sampler, begin, samples)]


@functools.lru_cache(maxsize=None)
def counts_of(name, begin=BEGIN, samples=SAMPLES):
    """the six counters of the case's annotation track over the oracle's lists (computed once per process)."""
    return E.model_counts(flat_of(cases()[name], ANNOTATOR), lists_of(name, ANNOTATOR, begin, samples), COUNTERS, samples)


def arrays(lists):
    """(segments, offsets) of (sample, unit) lists as gat_sample_units returns them."""
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return O.segs([x for l in lists for x in l]), off


def contig_lists(case, lists):
    """the contig-level lists gat_sample returns: a contig's units concatenated and merge(0)d (fromIsochores)."""
    flat = flat_of(case, ANNOTATOR, with_annos=False)
    n, nc = int(flat["n_units"]), int(flat["n_contigs"])
    out = []
    for s in range(len(lists) // n):
        contig = [[] for _ in range(nc)]
        for u in range(n):
            contig[int(flat["unit_contig"][u])] += lists[s * n + u]
        if int(flat["merge_contigs"]):
            contig = [O.aslist(O.merge(sorted(x), 0)) if x else [] for x in contig]
        out += contig
    return out


def min_used(name, sampler=ANNOTATOR):
    return min(st.used for st in streams_of(name, sampler))


def need_more(name, rows, sampler=ANNOTATOR):
    """the streams of the case's call that need more than `rows` outputs by the device's count"""
    return sum(st.used > rows for st in streams_of(name, sampler))


# ------------------------------------------------------------------------------------------------ the sweep tables
# A table holds TARGET ROWS (multiples of 16).  MAX_ROWS[case]: no sweep asks the case for more rows than this, and every
# stream of the case's call needs more outputs than this (asserted in tests/test_rows_cases_model.py): at every target of
# a sweep all 70 streams run out.
MAX_ROWS = {"small": 144, "small_b3": 144, "mid": 768, "mid_simple": 800, "mid_grid": 704, "large": 2480, "long": 2048}
MAX_ROWS_SEGMENTS = {"small": 144, "mid": 736}

# mid: every value of rows % 624 -- 64..608 as they are, 0..48 as 624..672 (a unit of 250 segments keeps a spread term of
# some thirty rows: 16 and 32 rows may not be within reach); in groups of about eight per test item
RESIDUE_ROWS = list(range(64, 688, 16))
RESIDUE_GROUPS = [RESIDUE_ROWS[i:i + 8] for i in range(0, len(RESIDUE_ROWS), 8)]
# large: rows / 624 in {1, 2, 3}, each at rows % 624 in {0, 16, 608}: the blocks rng_switch twists; pos = 0 (tempering left
# to rng_next), right behind it, and the partial last block of 64 (lanes clamped at word 623)
BLOCK_ROWS = [MT_N * b + r for b in (1, 2, 3) for r in (0, 16, 608)]
BLOCK_GROUPS = [BLOCK_ROWS[0:3], BLOCK_ROWS[3:6], BLOCK_ROWS[6:9]]
# small, small_b3: rows is exact
SMALL_ROWS = [16, 32, 48, 64, 80, 128, 144]
# the routes: three row counts deep in placement, about a quarter of the shortest stream (the placement kernels hand over -3;
# 192 is a multiple of 64, 176 and 208 are not), and three just under the shortest stream -- mid: at 768 nearly every stream
# is past its first consolidation, at 752 some, at 736 none (they hand over -3 with nearly the whole list placed);
# mid_simple: at all three every stream is past it
ROUTE_ROWS_DEEP = [176, 192, 208]
ROUTE_ROWS_LATE = {"mid": [736, 752, 768], "mid_simple": [768, 784, 800]}
# mid: between a quarter and three quarters of the streams need more (tests/test_rows_cases_model.py)
MIXED_ROWS = 800
# the short budget of the tests that are about something else than the switch position: deep in placement
SHORT_ROWS = {"small": 48, "small_b3": 48, "mid": 208, "mid_simple": 208, "mid_grid": 208, "large": 640, "long": 1040}
# long: a budget that ends behind the first consolidation of some streams (k_tail_big / k_resume_big run out: no generator
# there, the unit is redone from its seed), within the placements of others, and that is enough for the rest
LONG_LATE_ROWS = 4832
