"""k_consolidate's bucket sort (wave_sort_bucket_sparse: lists of 65..512 placed segments, every element written once, only
buckets of two or more members sorted) against the oracle, at the borders of its paths and where keys collide.

One unit per problem, 64 or 128 samples (one or two tiles of k_place / k_tail).  The list k_consolidate sorts is what k_place
placed up to the first consolidation: about as many segments as the unit has, a few more or fewer from sample to sample, so
a spread of segment counts around 64/65 (register network | bucket sort, 512 buckets), 256/257 (512 | 1 024 buckets) and
512/513 (| the counting sort of 513..1 024) puts lists on both sides of every border.

Which kernel finishes a unit: k_consolidate takes EVERY unit of these problems (lists within its LDS); k_tail finishes the unit
unless a segment placed behind the first consolidation touches the merged list, a second trim is needed or more than four
segments are placed -- then k_sampler resumes it FROM k_consolidate's merged list (n_queued_units).  A unit run in full by
k_sampler (n_full_units) would bypass k_consolidate: none may be.  What k_tail leaves on spread-out lists (DESIGN §10 has the
reasons counted on config 2: 2.5 % of the units): a fifth new segment -- the overlaps among n placed segments covering a share c
of their workspace cost about n c / 2 segments' worth of bases, placed again behind the consolidation: c = 0.2 % keeps that
below one for n <= 521, a fifth is then rarer than one unit in a hundred --, a new segment that touches the list (2 c per
placement) and a trim that walks over more than six segments (a per cent or two on config 2, whose lengths vary as much).  A
few per cent in all; with 64 samples a share of 5 % has a standard deviation of 2.7 %: MAX_QUEUED = 0.15 is beyond three of
them.  The crowded cases (a sixth to a third of the workspace covered) are k_sampler's for the most part by
design; there only n_full_units == 0 and the consolidation's result are asserted."""
import functools

import numpy as np
import pytest

from gat_amd import _lib
from oracle import oracle as O

COUNTERS = ["nucleotide-overlap", "segment-overlap"]
SEED = 77
MAX_QUEUED = 0.15


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0)
    yield c
    c.close()


def _flat(segments, workspace):
    s, w = O.segs(segments), O.segs(workspace)
    return dict(n_units=1, segs=s, seg_off=[0, len(s)], ws=w, ws_off=[0, len(w)], unit_contig=[0], n_contigs=1,
                merge_contigs=0, n_tracks=1, annos=w, anno_off=[0, len(w)], cws_nseg=[len(w)],
                bucket_size=1, nbuckets=100000)


def _spread(n, seed, coverage=0.002, lo=20, hi=200):
    """n segments of lo..hi bases on one workspace piece they cover `coverage` of"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(lo, hi + 1, size=n)
    size = int(lens.sum() / coverage)
    starts = np.sort(rs.choice(size // (hi + 1), size=n, replace=False)) * (hi + 1)
    return [(int(s), int(s + l)) for s, l in zip(starts, lens)], [(0, size)]


def _short(n, seed, lo, hi, origin=1000):
    """n segments of lo..hi bases side by side from `origin` on (inside the first workspace piece: the sampler only takes
    segments that touch the workspace)"""
    rs = np.random.RandomState(seed)
    lens = rs.randint(lo, hi + 1, size=n)
    starts = origin + np.arange(n) * (hi + 1)
    return [(int(s), int(s + l)) for s, l in zip(starts, lens)]


def _cases():
    c = {}
    # path borders: placed lists around 64/65, 256/257, 512/513
    for border in (64, 256, 512):
        for n in (border - 7, border - 3, border - 1, border, border + 1, border + 2, border + 5, border + 9):
            c["border%d_n%d" % (border, n)] = _spread(n, 1000 + n) + (64, True)
    # every bucket a singleton (nearly): few segments on a huge workspace
    segs, _ = _spread(90, 5, coverage=0.5)
    c["singletons"] = (segs, [(0, 2000000000)], 128, True)                    # (the segments lie inside it)
    c["spread400"] = _spread(400, 6) + (128, True)
    # heavy collision: two short pieces far apart -- two crowded buckets, the rest empty: beyond the cap, the network --
    # and less far apart: ~20 buckets per piece with ~7 members each, most lists under the cap of 16
    c["collide_cap"] = (_short(300, 7, 1, 5), [(1000, 4000), (1500000000, 1500003000)], 64, False)
    c["collide_crowded"] = (_short(300, 8, 1, 5), [(1000, 4000), (150000, 153000)], 64, False)
    c["collide_crowded200"] = (_short(200, 9, 1, 5), [(1000, 3000), (80000, 82000)], 64, False)
    # a mix: a long piece (39 of 1 024 buckets, ~7 members each) beside fifty fragments a bucket apart or more (0..3 each)
    segs, _ = _spread(400, 10, lo=20, hi=100)        # (0.4 % of the 6 Mb)
    c["mix"] = (segs, [(0, 4000000)] + [(5000000 + 2000000 * k, 5040000 + 2000000 * k) for k in range(50)], 64, True)
    # span below the bucket count: `direct` buckets, many equal starts with different ends
    c["direct512"] = (_short(110, 11, 1, 3), [(1000, 1500)], 64, False)
    c["direct1024"] = (_short(300, 12, 1, 1), [(1000, 1900)], 64, False)
    # (all starts equal -- span 0 -- is not among the cases: a placement's start only repeats at the clamp to position 0, and more
    #  than 64 segments that all land there need more than 64 segments touching one short workspace piece at 0, which only copies
    #  of one segment can: the oracle refuses such a list (its assertion, not a ValueError).  The sort returns to the network for
    #  span 0 before it touches LDS, as wave_sort_bucket does; direct512 / direct1024 have the runs of equal starts)
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def _reference(name):
    """(flat, counts, (segments, offsets)) of the oracle: computed once per case, shared, never modified"""
    segs, ws, S, _ = CASES[name]
    flat = _flat(segs, ws)
    want, wsamples = O.run_samples(flat, COUNTERS, SEED, 1, 0, S, want_samples=True)
    for a in want + list(wsamples):
        a.setflags(write=False)
    return flat, want, wsamples


def test_inputs_are_valid_for_the_reference():
    """the oracle alone (no GPU): none of the inputs raises the reference's ValueError, and the lists have the lengths
    the cases are about"""
    for name in CASES:
        flat, want, (seg, off) = _reference(name)
        assert len(off) == CASES[name][2] + 1 and len(seg) > 0, name


def _check(ctx, name):
    segs, ws, S, spread = CASES[name]
    flat, want, (wseg, woff) = _reference(name)
    P = _lib.Problem(ctx, flat)
    try:
        got = P.sample_and_count(COUNTERS, SEED, 0, S)
        st = P.last_stats
        for k, c in enumerate(COUNTERS):
            assert np.array_equal(got[k], want[k]), (name, c)
        seg, off = P.sample(SEED, 0, S)
        st2 = P.last_stats
        assert np.array_equal(off, woff) and np.array_equal(seg, wseg), name
    finally:
        P.close()
    for s in (st, st2):
        queued = s["n_queued_units"] / float(S)
        print("%s: n_tail_units %d, n_queued_units %d (%.3f), n_full_units %d, n_resumed_units %d"
              % (name, s["n_tail_units"], s["n_queued_units"], queued, s["n_full_units"], s["n_resumed_units"]))
        # the split path took the units: nothing bypassed k_consolidate, and what k_tail did not finish was resumed from its list
        assert s["n_full_units"] == 0, name
        assert s["n_tail_units"] + s["n_queued_units"] == S, name
        if spread:
            assert s["n_tail_units"] > 0 and queued <= MAX_QUEUED, (name, queued)


@pytest.mark.gpu
@pytest.mark.parametrize("border", [64, 256, 512])
def test_path_borders(ctx, border):
    for name in sorted(CASES):
        if name.startswith("border%d_" % border):
            _check(ctx, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["singletons", "spread400", "collide_cap", "collide_crowded", "collide_crowded200", "mix",
                                  "direct512", "direct1024"])
def test_collisions(ctx, name):
    _check(ctx, name)
